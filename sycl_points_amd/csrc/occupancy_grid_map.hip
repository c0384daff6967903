// OccupancyGridMap for gfx950 — the log-odds submap of Submap::build_submap (replaces mapping/occupancy_grid_map.hpp:27-472,
// 482-1687).
//
// The table is sp_voxel_table.h's, as VoxelHashMap's, with 128 probes, a `deleted` key for pruned slots and a 32-byte core {sum xyz,
// log_odds, hit_count, miss_count, and the part of either count already applied to log_odds}; the host state, the compaction
// scratch and the overlap kernel are there too.
// add_point_cloud is the reference's five steps: [rehash] -> hits, one lane per point -> carving, one lane per ray -> apply -> prune.
// extract_visible_points (:183-411) is two passes with a compaction between them and one after: candidate flags, one lane per slot
// (occupied, within max_distance, inside the frustum) -> scan -> the candidates' slots as a dense list -> the occlusion walk, one lane
// per candidate, which clears the flag of a candidate it finds occluded -> scan -> rows. The walk reads the table and writes nothing
// to it; it is the carving kernel's counted walk with another visitor (counted_walk below).
// Where this differs from the reference, on purpose:
//   * the ray walk is a counted loop of exactly |dix| + |diy| + |diz| steps in which an axis that has reached the target's cell no
//     longer competes; the reference's `while (true)` (:880-899) ends only by landing on the target cell;
//   * rays that end at a non-finite point or outside the 21-bit cell range post nothing, and neither does a frame whose sensor sits
//     outside that range (the reference casts NaN to int64 / walks millions of rejected cells);
//   * pending log-odds are two integer counts per voxel, turned into hits * log_hit + misses * log_miss by the apply kernel, so the
//     log-odds do not depend on the order in which lanes arrive (the reference adds floats with relaxed atomics: order unspecified);
//   * a pruned slot's covariance sums are cleared with the rest (the reference leaves them to whoever claims the slot next);
//   * extract_visible_points: the two cosines of the frustum test are forward / sqrtf(norm_sq), both correctly rounded, where the
//     reference multiplies by sycl::rsqrt (implementation-defined); rows come out in table-slot order (the reference hands them out
//     through an atomic counter); a sensor at a non-finite position or outside the 21-bit cell range sees nothing; other
//     non-finite arguments are refused.
// The walk's arithmetic is IEEE multiply / subtract / add / floor / one division per axis, compiled uncontracted (-ffp-contract=off,
// csrc/Makefile) with hipcc's correctly rounded division: the cells are those of tests/cpp/occupancy_grid_restate.cpp bit for bit.

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "sp_voxel_table.h"

namespace sp {
namespace {

constexpr uint64_t kDeletedKey = ~0ull - 1;  // VoxelConstants::deleted_coord
constexpr unsigned kOgmMaxProbe = 128;       // occupancy_grid_map.hpp:1679
constexpr int kCellOffset = 1 << 20, kCellMask = (1 << 21) - 1;

struct OgmCore {  // 32 bytes
    float sx, sy, sz, log_odds;
    uint32_t hit_count, miss_count;        // totals since the voxel was claimed
    uint32_t hits_applied, misses_applied; // the part of the totals log_odds already holds
};

using OgmTable = VoxelTable<OgmCore>;

__device__ __forceinline__ bool live(uint64_t k) { return k != kInvalidKey && k != kDeletedKey; }

// grid_to_key_device (:903-920)
__device__ __forceinline__ uint64_t cell_key(int x, int y, int z) {
    const int cx = x + kCellOffset, cy = y + kCellOffset, cz = z + kCellOffset;
    if (cx < 0 || cx > kCellMask || cy < 0 || cy > kCellMask || cz < 0 || cz > kCellMask) return kInvalidKey;
    return (uint64_t)cx | ((uint64_t)cy << 21) | ((uint64_t)cz << 42);
}

// The slot search of global_reduction (:795-818): the first free or pruned slot is claimed with one compare-and-swap; a swap that
// loses to the same key uses that slot, one that loses to another key moves on with the probe loop. Never more than kOgmMaxProbe
// probes and never a second swap on one slot; an entry that finds no slot is dropped, as in the reference.
// Not VoxelHashMap's insert(), on purpose: this one loads first, probes 128 times and reuses `deleted` slots.
__device__ __forceinline__ unsigned long long find_or_claim(const OgmTable& t, uint64_t h, unsigned* __restrict__ voxel_num) {
    for (unsigned p = 0; p < kOgmMaxProbe; ++p) {
        const unsigned long long s = slot_id(h, p, t.capacity);
        unsigned long long* kp = reinterpret_cast<unsigned long long*>(t.key + s);
        unsigned long long seen = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == kInvalidKey || seen == kDeletedKey) {
            const unsigned long long prev = atomicCAS(kp, seen, (unsigned long long)h);
            if (prev == seen) { atomicAdd(voxel_num, 1u); return s; }
            seen = prev;
        }
        if (seen == h) return s;
    }
    return kNoSlot;
}

// integrate_points (:1072-1233): load_entry + global_reduction, one lane per point. The reference's work-group pre-combination of
// equal keys is not done (as in voxel_hash_map.hip; not measured for this map).
__global__ __launch_bounds__(kBlock) void ogm_hit_kernel(OgmTable t, const float4* __restrict__ pts, const float4* __restrict__ covs,
                                                         const float4* __restrict__ rgb, const float* __restrict__ inten,
                                                         unsigned n, Mat4Arg pose, float inv, bool map_has_cov, bool map_has_rgb,
                                                         bool map_has_intensity, uint32_t frame,
                                                         unsigned* __restrict__ voxel_num) {
    const Rigid T = load_rigid_colmajor(pose.m);
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const float4 p = pts[i];
        float wx, wy, wz;
        transform_point(T, p.x, p.y, p.z, wx, wy, wz);
        const uint64_t h = voxel_key3(wx, wy, wz, inv);
        if (h == kInvalidKey) continue;
        const unsigned long long s = find_or_claim(t, h, voxel_num);
        if (s == kNoSlot) continue;
        OgmCore* c = t.core + s;
        fadd(&c->sx, wx);
        fadd(&c->sy, wy);
        fadd(&c->sz, wz);
        atomicAdd(&c->hit_count, 1u);
        if (map_has_cov && covs) add_cov_sums(t, s, encode_cov(covs + 4 * (size_t)i, T));
        if (map_has_rgb && rgb) add_color_sums(t, s, rgb[i]);
        if (map_has_intensity && inten) fadd(t.intensity + s, inten[i]);
        stamp(t, s, frame);  // :806, 815
    }
}

// What a ray is, for the estimate and the walk alike: its end point in the map frame, the end point's cell, and whether it is cast.
struct Ray {
    float wx, wy, wz;
    int tx, ty, tz;
    bool cast;
};
// the ray to a map-frame point: cast when the point has a cell (finite, inside the 21-bit range)
__device__ __forceinline__ Ray ray_to(float wx, float wy, float wz, float inv) {
    Ray r;
    r.wx = wx; r.wy = wy; r.wz = wz;
    r.tx = r.ty = r.tz = 0;
    r.cast = voxel_key3(wx, wy, wz, inv) != kInvalidKey;
    if (!r.cast) return r;
    r.tx = (int)floorf(wx * inv);
    r.ty = (int)floorf(wy * inv);
    r.tz = (int)floorf(wz * inv);
    return r;
}
__device__ __forceinline__ Ray make_ray(const Rigid& T, const float4 p, float ox, float oy, float oz, float inv) {
    float wx, wy, wz;
    transform_point(T, p.x, p.y, p.z, wx, wy, wz);
    Ray r = ray_to(wx, wy, wz, inv);  // non-finite or outside the 21-bit range: skipped whole
    if (!r.cast) return r;
    const float dx = wx - ox, dy = wy - oy, dz = wz - oz;
    const float dist_sq = dx * dx + dy * dy + dz * dz;
    if (dist_sq <= FLT_EPSILON) r.cast = false;  // :1306, 1400
    return r;
}

// Where every ray of a call starts: the sensor position in cell units, its floor and its cell (inside the 21-bit range: the host
// checked).
struct WalkOrigin {
    float sox, soy, soz, fox, foy, foz;
    int oix, oiy, oiz;
};
__device__ __forceinline__ WalkOrigin walk_origin(float ox, float oy, float oz, float inv) {
    WalkOrigin o;
    o.sox = ox * inv; o.soy = oy * inv; o.soz = oz * inv;
    o.fox = floorf(o.sox); o.foy = floorf(o.soy); o.foz = floorf(o.soz);
    o.oix = (int)o.fox; o.oiy = (int)o.foy; o.oiz = (int)o.foz;
    return o;
}
__device__ __forceinline__ unsigned walk_steps(const WalkOrigin& o, const Ray& r) {
    return (unsigned)(abs(r.tx - o.oix) + abs(r.ty - o.oiy) + abs(r.tz - o.oiz));
}

// The walk of traverse_ray_exclusive_impl (:823-900) as a counted loop: exactly steps = |dix| + |diy| + |diz| steps, each along an
// axis that has not reached the target's cell yet — the smallest t_max among those, ties to x then y, as the reference orders its
// comparisons. Wherever the reference's loop ends this visits its cells in its order. visit(key) is called for every cell stepped
// into but the last (the target's own cell is excluded) and ends the walk by returning false.
template <class Visit>
__device__ __forceinline__ void counted_walk(const WalkOrigin& o, const Ray& r, float inv, unsigned steps, Visit visit) {
    const float inf = INFINITY;
    int ix = o.oix, iy = o.oiy, iz = o.oiz;
    const float dir_x = r.wx * inv - o.sox, dir_y = r.wy * inv - o.soy, dir_z = r.wz * inv - o.soz;
    const float ax = fabsf(dir_x), ay = fabsf(dir_y), az = fabsf(dir_z);
    const int step_x = (dir_x > 0.0f) ? 1 : ((dir_x < 0.0f) ? -1 : 0);
    const int step_y = (dir_y > 0.0f) ? 1 : ((dir_y < 0.0f) ? -1 : 0);
    const int step_z = (dir_z > 0.0f) ? 1 : ((dir_z < 0.0f) ? -1 : 0);
    const float frac_x = o.sox - o.fox, frac_y = o.soy - o.foy, frac_z = o.soz - o.foz;
    const float inv_x = (ax > FLT_EPSILON) ? (1.0f / ax) : inf;
    const float inv_y = (ay > FLT_EPSILON) ? (1.0f / ay) : inf;
    const float inv_z = (az > FLT_EPSILON) ? (1.0f / az) : inf;
    float t_max_x = (step_x != 0) ? ((step_x > 0 ? (1.0f - frac_x) : frac_x) * inv_x) : inf;
    float t_max_y = (step_y != 0) ? ((step_y > 0 ? (1.0f - frac_y) : frac_y) * inv_y) : inf;
    float t_max_z = (step_z != 0) ? ((step_z > 0 ? (1.0f - frac_z) : frac_z) * inv_z) : inf;
    const float t_delta_x = (step_x != 0) ? inv_x : inf;
    const float t_delta_y = (step_y != 0) ? inv_y : inf;
    const float t_delta_z = (step_z != 0) ? inv_z : inf;
    // An axis whose cells differ has a non-zero direction of the right sign (floor is monotone), so step_* leads to the target.
    for (unsigned s = 1; s <= steps; ++s) {
        const bool ux = ix != r.tx, uy = iy != r.ty, uz = iz != r.tz;  // axes still short of the target: at least one
        int axis;
        if (ux && (!uy || t_max_x <= t_max_y) && (!uz || t_max_x <= t_max_z)) axis = 0;
        else if (uy && (!uz || t_max_y <= t_max_z)) axis = 1;
        else if (uz) axis = 2;
        else axis = uy ? 1 : 0;  // only reached through a NaN t_max (0 * inf): still an axis that is short
        if (axis == 0) { ix += step_x; t_max_x += t_delta_x; }
        else if (axis == 1) { iy += step_y; t_max_y += t_delta_y; }
        else { iz += step_z; t_max_z += t_delta_z; }
        if (s == steps) break;  // the target's cell itself is excluded
        if (!visit(cell_key(ix, iy, iz))) break;  // between two cells inside the range the key is always valid
    }
}

// The origin-voxel hit flag (:1258-1280) and the visit estimate (:1283-1335) in one pass: out[0..1] = the estimate (64 bits),
// out[2] = 1 when a point of the cloud lies in the sensor's own cell.
__global__ __launch_bounds__(kBlock) void ogm_estimate_kernel(const float4* __restrict__ pts, unsigned n, Mat4Arg pose, float inv,
                                                              float ox, float oy, float oz, int oix, int oiy, int oiz,
                                                              uint64_t origin_key, unsigned* __restrict__ out) {
    const Rigid T = load_rigid_colmajor(pose.m);
    unsigned visits = 0, hit = 0;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const float4 p = pts[i];
        const Ray r = make_ray(T, p, ox, oy, oz, inv);
        if (voxel_key3(r.wx, r.wy, r.wz, inv) == origin_key) hit = 1;  // origin_key is a valid key here
        if (!r.cast) continue;
        const unsigned steps = (unsigned)(abs(r.tx - oix) + abs(r.ty - oiy) + abs(r.tz - oiz));
        visits += steps > 0 ? steps + 1 : 0;  // the origin cell plus the traversed cells (:1331); at most 3 * 2^21 + 1 per ray
    }
    // a lane's own sum can wrap only beyond 2^32 / (3 * 2^21) = 682 rays of the longest possible length per lane: summed in 64 bits
    unsigned long long total = visits;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) total += (unsigned long long)__shfl_xor((long long)total, o, 64);
    hit = wave_sum_u32(hit);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (total) atomicAdd(reinterpret_cast<unsigned long long*>(out), total);
        if (hit) atomicMax(out + 2, 1u);
    }
}

__device__ __forceinline__ void post_miss(const OgmTable& t, uint64_t key, uint32_t frame, unsigned* __restrict__ voxel_num) {
    const unsigned long long s = find_or_claim(t, key, voxel_num);
    if (s == kNoSlot) return;
    atomicAdd(&t.core[s].miss_count, 1u);
    stamp(t, s, frame);
}

// update_free_space's walk (:1385-1448), one lane per ray: counted_walk with a visitor that posts a miss and never stops.
__global__ __launch_bounds__(kBlock) void ogm_walk_kernel(OgmTable t, const float4* __restrict__ pts, unsigned n, Mat4Arg pose,
                                                          float inv, float ox, float oy, float oz, bool skip_origin_miss,
                                                          uint32_t frame, unsigned* __restrict__ voxel_num) {
    const Rigid T = load_rigid_colmajor(pose.m);
    const WalkOrigin o = walk_origin(ox, oy, oz, inv);
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const float4 p = pts[i];
        const Ray r = make_ray(T, p, ox, oy, oz, inv);
        if (!r.cast) continue;
        const unsigned steps = walk_steps(o, r);
        if (steps == 0) continue;  // the hit lies in the sensor's own cell
        if (!skip_origin_miss) post_miss(t, cell_key(o.oix, o.oiy, o.oiz), frame, voxel_num);  // :1427-1433
        counted_walk(o, r, inv, steps, [&](uint64_t key) {
            if (key != kInvalidKey) post_miss(t, key, frame, voxel_num);
            return true;
        });
    }
}

// apply_pending_log_odds (:1457-1483) with the pending value formed here from the two counts
__global__ __launch_bounds__(kBlock) void ogm_apply_kernel(OgmTable t, float log_hit, float log_miss, float lo_min, float lo_max) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= t.capacity || !live(t.key[i])) return;
    OgmCore c = t.core[i];
    const uint32_t h = c.hit_count - c.hits_applied, m = c.miss_count - c.misses_applied;
    if (h == 0 && m == 0) return;
    const float delta = (float)h * log_hit + (float)m * log_miss;
    if (delta != 0.0f) c.log_odds = fmaxf(lo_min, fminf(lo_max, c.log_odds + delta));
    c.hits_applied = c.hit_count;
    c.misses_applied = c.miss_count;
    t.core[i] = c;
}

// prune_stale_voxels (:1485-1528)
__global__ __launch_bounds__(kBlock) void ogm_prune_kernel(OgmTable t, uint32_t frame, uint32_t stale_threshold,
                                                           unsigned* __restrict__ voxel_num) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= t.capacity || !live(t.key[i])) return;
    if ((frame - t.last_update[i]) > stale_threshold) {
        t.key[i] = kDeletedKey;
        t.core[i] = OgmCore{0, 0, 0, 0, 0, 0, 0, 0};
        t.cov[i] = CovSum{0, 0, 0, 0, 0, 0};
        t.color[i] = make_float4(0, 0, 0, 0);
        t.intensity[i] = 0.0f;
        t.last_update[i] = 0;
        return;
    }
    atomicAdd(voxel_num, 1u);
}

// rehash (:652-782): every live slot re-enters the new table through free slots only: claimed once, then copied.
// Not VoxelHashMap's rehash kernel, on purpose: that one merges entries of one key with atomic adds; this one, as the reference's,
// keeps them apart. A table can hold a key twice: find_or_claim takes the first `deleted` slot of the key's sequence before it reaches
// the key's own slot further along. Both entries move, the one that claims the earlier slot of the new sequence answers the lookups.
__global__ __launch_bounds__(kBlock) void ogm_rehash_kernel(OgmTable old_t, OgmTable new_t, bool has_cov, bool has_rgb,
                                                            bool has_intensity, unsigned* __restrict__ voxel_num) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= old_t.capacity) return;
    const uint64_t k = old_t.key[i];
    if (!live(k)) return;
    for (unsigned p = 0; p < kOgmMaxProbe; ++p) {
        const unsigned long long s = slot_id(k, p, new_t.capacity);
        if (atomicCAS(reinterpret_cast<unsigned long long*>(new_t.key + s), kInvalidKey, (unsigned long long)k) != kInvalidKey)
            continue;
        new_t.core[s] = old_t.core[i];
        if (has_cov) new_t.cov[s] = old_t.cov[i];
        if (has_rgb) new_t.color[s] = old_t.color[i];
        if (has_intensity) new_t.intensity[s] = old_t.intensity[i];
        new_t.last_update[s] = old_t.last_update[i];
        atomicAdd(voxel_num, 1u);
        return;
    }
}

// compute_overlap_ratio (:417-472) and the occluders of extract_visible_points (:332): a voxel counts when it was hit and is occupied
struct Occupied {
    float threshold;
    __device__ bool operator()(const OgmCore& c) const { return c.hit_count > 0u && !(c.log_odds < threshold); }
};

// flags for the two compactions: every live slot (export), or the occupied voxels near the sensor (:1568-1589).
// Each map's flag kernel tests its own condition: not shared.
__global__ __launch_bounds__(kBlock) void ogm_flag_kernel(OgmTable t, bool occupied_only, float threshold, float sx, float sy,
                                                          float sz, float max_dist, unsigned* __restrict__ flags) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= t.capacity) return;
    bool keep = live(t.key[i]);
    if (keep && occupied_only) {
        const OgmCore c = t.core[i];
        keep = c.hit_count != 0u && !(c.log_odds < threshold);
        if (keep) {
            const float inv = 1.0f / (float)c.hit_count;
            const float dx = fabsf(c.sx * inv - sx), dy = fabsf(c.sy * inv - sy), dz = fabsf(c.sz * inv - sz);
            keep = !(fmaxf(fmaxf(dx, dy), dz) > max_dist);
        }
    }
    flags[i] = keep ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void ogm_extract_kernel(OgmTable t, const unsigned* __restrict__ flags,
                                                             const unsigned* __restrict__ pos, unsigned out_capacity, MeanRows out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= t.capacity || !flags[i]) return;
    const unsigned o = pos[i];
    if (o >= out_capacity) return;
    const OgmCore c = t.core[i];
    write_mean_row(t, i, o, c.hit_count, c.sx, c.sy, c.sz, out);
}

// extract_visible_points, first pass (:250-311): flags[slot] = 1 for a candidate — an occupied voxel whose centroid lies within
// max_distance (L2) of the sensor and inside the frustum. local = R^T d is eigen_utils::multiply<3, 3> (one fma chain per row). The
// cosines are forward / sqrtf(norm_sq), not forward * rsqrt(norm_sq) as in the reference (:291, 305): division and square root are
// correctly rounded, sycl::rsqrt is implementation-defined.
struct Frustum {
    float sx, sy, sz;  // the sensor position
    float max_dist_sq, cos_limit_horizontal, cos_limit_vertical;
    bool include_backward;
};
__device__ __forceinline__ float clamp_unit(float c) { return c < -1.0f ? -1.0f : (c > 1.0f ? 1.0f : c); }

__global__ __launch_bounds__(kBlock) void ogm_visible_flag_kernel(OgmTable t, float threshold, Mat4Arg pose, Frustum f,
                                                                  unsigned* __restrict__ flags) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= t.capacity) return;
    bool keep = live(t.key[i]);
    if (keep) {
        const OgmCore c = t.core[i];
        keep = c.hit_count != 0u && !(c.log_odds < threshold);
        if (keep) {
            const Rigid T = load_rigid_colmajor(pose.m);
            const float inv = 1.0f / (float)c.hit_count;
            const float dx = c.sx * inv - f.sx, dy = c.sy * inv - f.sy, dz = c.sz * inv - f.sz;
            const float dist_sq = dx * dx + dy * dy + dz * dz;
            const float lx = chain3(T.R[0][0], dx, T.R[1][0], dy, T.R[2][0], dz);
            const float ly = chain3(T.R[0][1], dx, T.R[1][1], dy, T.R[2][1], dz);
            const float lz = chain3(T.R[0][2], dx, T.R[1][2], dy, T.R[2][2], dz);
            const float forward = f.include_backward ? fabsf(lx) : lx;  // :284: the limits apply behind the sensor as in front
            const float h_sq = forward * forward + ly * ly, v_sq = forward * forward + lz * lz;
            const float cos_h = h_sq > 0.0f ? clamp_unit(forward / sqrtf(h_sq)) : 1.0f;
            const float cos_v = v_sq > 0.0f ? clamp_unit(forward / sqrtf(v_sq)) : 1.0f;
            keep = dist_sq <= f.max_dist_sq && (f.include_backward || !(lx <= 0.0f)) && !(cos_h < f.cos_limit_horizontal) &&
                   !(cos_v < f.cos_limit_vertical);
        }
    }
    flags[i] = keep ? 1u : 0u;
}

// the flagged slots as a dense list in slot order: list[pos[slot]] = slot
__global__ __launch_bounds__(kBlock) void ogm_candidate_list_kernel(const unsigned* __restrict__ flags,
                                                                    const unsigned* __restrict__ pos, unsigned long long capacity,
                                                                    unsigned* __restrict__ list) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < capacity && flags[i]) list[pos[i]] = (unsigned)i;
}

// extract_visible_points, second pass (:313-361), one lane per candidate: the counted walk from the sensor to the candidate's
// centroid, stopped at the first occluder — another occupied voxel whose centroid is nearer to the sensor by more than 1e-6 in the
// squared distance (:341). An occluded candidate's flag is cleared. *count is the number of candidates (the scan's total, device
// memory); the host knows only its bound, voxel_num, and sizes the grid from that. Reads the table, writes nothing to it, no atomics.
__global__ __launch_bounds__(kBlock) void ogm_visible_walk_kernel(OgmTable t, const unsigned* __restrict__ list,
                                                                  const unsigned* __restrict__ count, float threshold, float ox,
                                                                  float oy, float oz, float inv, float voxel_size,
                                                                  unsigned* __restrict__ flags) {
    const unsigned n = *count;
    const WalkOrigin o = walk_origin(ox, oy, oz, inv);
    const Occupied occupied{threshold};
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const unsigned slot = list[i];
        const uint64_t own_key = t.key[slot];
        const OgmCore c = t.core[slot];
        const float inv_count = 1.0f / (float)c.hit_count;
        const float cx = c.sx * inv_count, cy = c.sy * inv_count, cz = c.sz * inv_count;
        const float dx = cx - ox, dy = cy - oy, dz = cz - oz;
        const float dist_sq = dx * dx + dy * dy + dz * dz;
        if (sqrtf(dist_sq) <= voxel_size) continue;  // :317: too near to be hidden
        const Ray r = ray_to(cx, cy, cz, inv);
        if (!r.cast) continue;  // a centroid without a cell (its sums overflowed): nothing to walk to
        bool occluded = false;
        counted_walk(o, r, inv, walk_steps(o, r), [&](uint64_t key) {
            if (key == kInvalidKey || key == own_key) return true;
            const unsigned long long s = find_slot<kOgmMaxProbe>(t.key, t.capacity, key);
            if (s == kNoSlot) return true;
            const OgmCore occ = t.core[s];
            if (!occupied(occ)) return true;
            const float inv_occ = 1.0f / (float)occ.hit_count;
            const float ex = occ.sx * inv_occ - ox, ey = occ.sy * inv_occ - oy, ez = occ.sz * inv_occ - oz;
            occluded = ex * ex + ey * ey + ez * ez + 1e-6f < dist_sq;
            return !occluded;
        });
        if (occluded) flags[slot] = 0u;
    }
}

__global__ __launch_bounds__(kBlock) void ogm_export_kernel(OgmTable t, const unsigned* __restrict__ flags,
                                                            const unsigned* __restrict__ pos, unsigned out_capacity,
                                                            uint64_t* __restrict__ keys, uint32_t* __restrict__ hits,
                                                            uint32_t* __restrict__ misses, float* __restrict__ log_odds,
                                                            uint32_t* __restrict__ last, float* __restrict__ xyz,
                                                            float* __restrict__ cov, float* __restrict__ rgb,
                                                            float* __restrict__ inten) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= t.capacity || !flags[i]) return;
    const size_t o = pos[i];
    if (o >= out_capacity) return;
    const OgmCore c = t.core[i];
    if (keys) keys[o] = t.key[i];
    if (hits) hits[o] = c.hit_count;
    if (misses) misses[o] = c.miss_count;
    if (log_odds) log_odds[o] = c.log_odds;
    if (last) last[o] = t.last_update[i];
    if (xyz) { xyz[3 * o] = c.sx; xyz[3 * o + 1] = c.sy; xyz[3 * o + 2] = c.sz; }
    if (cov) {
        const CovSum s = t.cov[i];
        float* d = cov + 6 * o;
        d[0] = s.xx; d[1] = s.xy; d[2] = s.xz; d[3] = s.yy; d[4] = s.yz; d[5] = s.zz;
    }
    if (rgb) {
        const float4 k = t.color[i];
        float* d = rgb + 4 * o;
        d[0] = k.x; d[1] = k.y; d[2] = k.z; d[3] = k.w;
    }
    if (inten) inten[o] = t.intensity[i];
}

// find_voxel (:591-609) for one key: out[0] = 1 and out[1] = the log-odds' bits when the map holds the voxel
__global__ void ogm_lookup_kernel(OgmTable t, uint64_t key, unsigned* __restrict__ out) {
    const unsigned long long s = find_slot<kOgmMaxProbe>(t.key, t.capacity, key);
    out[0] = s != kNoSlot;
    out[1] = s != kNoSlot ? __float_as_uint(t.core[s].log_odds) : 0u;
}

}  // namespace
}  // namespace sp

struct sp_occupancy_grid_map : sp::VoxelMapState<sp::OgmCore> {  // defaults: occupancy_grid_map.hpp:1658-1680
    float log_odds_hit = 0.85f, log_odds_miss = -0.4f, min_log_odds = -4.0f, max_log_odds = 4.0f;
    float occupancy_probability = 0.5f, occupancy_threshold_log_odds = 0.0f;  // log(0.5 / (1 - 0.5))
    bool free_space_updates = true, voxel_pruning = true;
    uint32_t frame_index = 0, stale_frame_threshold = 100;
    // the counter beyond its first word: the lookup's result takes two, the visit estimate (64 bits) + origin hit three
};

namespace sp {
namespace {

auto rehash_launch(const sp_occupancy_grid_map* m, hipStream_t st) {
    return [=](const OgmTable& old_t, const OgmTable& new_t) {
        ogm_rehash_kernel<<<div_up(old_t.capacity, kBlock), kBlock, 0, st>>>(old_t, new_t, m->has_cov, m->has_rgb, m->has_intensity,
                                                                            m->counter);
    };
}

float probability_to_log_odds(float p) { return std::log(p / (1.0f - p)); }  // :559-561

// the slot-order compaction both exports use, up to the scan
int flag_and_scan(sp_occupancy_grid_map* m, bool occupied_only, const float* sensor3, float max_distance, hipStream_t st) {
    int rc = m->ensure_scratch();
    if (rc != SP_OK) return rc;
    ogm_flag_kernel<<<div_up((size_t)m->t.capacity, kBlock), kBlock, 0, st>>>(
        m->t, occupied_only, m->occupancy_threshold_log_odds, sensor3 ? sensor3[0] : 0.0f, sensor3 ? sensor3[1] : 0.0f,
        sensor3 ? sensor3[2] : 0.0f, max_distance, m->flags);
    return m->scan_flags(st);
}

// update_free_space (:1235-1455)
int carve(sp_occupancy_grid_map* m, const float4* pts, unsigned n, const float* pose16, hipStream_t st) {
    const float ox = pose16 ? pose16[12] : 0.0f, oy = pose16 ? pose16[13] : 0.0f, oz = pose16 ? pose16[14] : 0.0f;
    const float inv = m->voxel_size_inv;
    const float fx = std::floor(ox * inv), fy = std::floor(oy * inv), fz = std::floor(oz * inv);
    const float lim = (float)kCellOffset;
    // a sensor outside the 21-bit cell range (or at a non-finite position): nothing is carved
    if (!(fx >= -lim && fx < lim && fy >= -lim && fy < lim && fz >= -lim && fz < lim)) return SP_OK;
    const int oix = (int)fx, oiy = (int)fy, oiz = (int)fz;
    const uint64_t origin_key = (uint64_t)(oix + kCellOffset) | ((uint64_t)(oiy + kCellOffset) << 21) |
                                ((uint64_t)(oiz + kCellOffset) << 42);
    int rc = m->write_counter(st, 0, 0, 0);
    if (rc != SP_OK) return rc;
    const Mat4Arg pose = pose_arg(pose16);
    ogm_estimate_kernel<<<stream_grid(n), kBlock, 0, st>>>(pts, n, pose, inv, ox, oy, oz, oix, oiy, oiz, origin_key, m->counter);
    unsigned est[3] = {0, 0, 0};
    rc = launch_status();
    if (rc == SP_OK) rc = m->read_counter(st, est, 3);
    if (rc != SP_OK) return rc;
    const unsigned long long expected = (unsigned long long)est[0] | ((unsigned long long)est[1] << 32);
    if (expected == 0) return SP_OK;  // :1343-1346
    // the growth loop (:1348-1355) climbs the ladder one rehash at a time; its last rung is reached here in one
    const float required = (float)(m->voxel_num + expected);
    size_t cap = (size_t)m->t.capacity;
    while (m->rehash_threshold < required / (float)cap) {
        const size_t next = next_capacity(cap);
        if (next <= cap) break;
        cap = next;
    }
    if ((rc = m->grow(cap, st, rehash_launch(m, st))) != SP_OK) return rc;
    if ((rc = m->write_counter(st, (unsigned)m->voxel_num)) != SP_OK) return rc;
    ogm_walk_kernel<<<stream_grid(n), kBlock, 0, st>>>(m->t, pts, n, pose, inv, ox, oy, oz, est[2] != 0, m->frame_index, m->counter);
    return m->read_voxel_num(st);
}

}  // namespace
}  // namespace sp

extern "C" int sp_ogm_create(float voxel_size, void* stream, sp_occupancy_grid_map** out) {
    return sp::create_map(voxel_size, stream, out);
}
extern "C" void sp_ogm_destroy(sp_occupancy_grid_map* m) { sp::destroy_map(m); }

extern "C" int sp_ogm_clear(sp_occupancy_grid_map* m, void* stream) {  // :42-69
    if (!m) return SP_ERR_INVALID_ARGUMENT;
    const int rc = m->reset_to_first_capacity(sp::as_stream(stream));
    if (rc == SP_OK) m->frame_index = 0;
    return rc;
}

extern "C" int sp_ogm_set_log_odds_limits(sp_occupancy_grid_map* m, float minimum, float maximum) {  // :107-113
    if (!m) return SP_ERR_INVALID_ARGUMENT;
    if (minimum > maximum) { sp_set_error("minimum must not exceed maximum."); return SP_ERR_INVALID_ARGUMENT; }
    m->min_log_odds = minimum;
    m->max_log_odds = maximum;
    return SP_OK;
}

extern "C" int sp_ogm_set(sp_occupancy_grid_map* m, int param, float value) {
    if (!m) return SP_ERR_INVALID_ARGUMENT;
    switch (param) {
        case SP_OGM_VOXEL_SIZE:
            if (!(value > 0.0f)) { sp_set_error("voxel_size must be positive."); return SP_ERR_INVALID_ARGUMENT; }
            m->voxel_size = value;
            m->voxel_size_inv = 1.0f / value;
            return SP_OK;
        case SP_OGM_LOG_ODDS_HIT: m->log_odds_hit = value; return SP_OK;
        case SP_OGM_LOG_ODDS_MISS: m->log_odds_miss = value; return SP_OK;
        case SP_OGM_LOG_ODDS_MIN: return sp_ogm_set_log_odds_limits(m, value, m->max_log_odds);
        case SP_OGM_LOG_ODDS_MAX: return sp_ogm_set_log_odds_limits(m, m->min_log_odds, value);
        case SP_OGM_OCCUPANCY_THRESHOLD:  // :116-121
            if (!(value > 0.0f) || !(value < 1.0f)) {
                sp_set_error("probability must be between 0 and 1.");
                return SP_ERR_INVALID_ARGUMENT;
            }
            m->occupancy_probability = value;
            m->occupancy_threshold_log_odds = sp::probability_to_log_odds(value);
            return SP_OK;
        case SP_OGM_FREE_SPACE_UPDATES: m->free_space_updates = value != 0.0f; return SP_OK;
        case SP_OGM_VOXEL_PRUNING: m->voxel_pruning = value != 0.0f; return SP_OK;
        case SP_OGM_STALE_FRAME_THRESHOLD: m->stale_frame_threshold = (uint32_t)value; return SP_OK;
        case SP_OGM_REHASH_THRESHOLD: m->rehash_threshold = value; return SP_OK;
    }
    return SP_ERR_INVALID_ARGUMENT;
}
extern "C" float sp_ogm_get(const sp_occupancy_grid_map* m, int param) {
    if (!m) return 0.0f;
    switch (param) {
        case SP_OGM_VOXEL_SIZE: return m->voxel_size;
        case SP_OGM_LOG_ODDS_HIT: return m->log_odds_hit;
        case SP_OGM_LOG_ODDS_MISS: return m->log_odds_miss;
        case SP_OGM_LOG_ODDS_MIN: return m->min_log_odds;
        case SP_OGM_LOG_ODDS_MAX: return m->max_log_odds;
        case SP_OGM_OCCUPANCY_THRESHOLD: return m->occupancy_probability;
        case SP_OGM_FREE_SPACE_UPDATES: return m->free_space_updates ? 1.0f : 0.0f;
        case SP_OGM_VOXEL_PRUNING: return m->voxel_pruning ? 1.0f : 0.0f;
        case SP_OGM_STALE_FRAME_THRESHOLD: return (float)m->stale_frame_threshold;
        case SP_OGM_REHASH_THRESHOLD: return m->rehash_threshold;
    }
    return 0.0f;
}
extern "C" size_t sp_ogm_info(const sp_occupancy_grid_map* m, int what) {
    if (!m) return 0;
    switch (what) {
        case SP_OGM_INFO_VOXEL_NUM: return m->voxel_num;
        case SP_OGM_INFO_CAPACITY: return (size_t)m->t.capacity;
        case SP_OGM_INFO_FRAME_INDEX: return m->frame_index;
        case SP_OGM_INFO_HAS_COV: return m->has_cov;
        case SP_OGM_INFO_HAS_RGB: return m->has_rgb;
        case SP_OGM_INFO_HAS_INTENSITY: return m->has_intensity;
    }
    return 0;
}

// add_point_cloud (:129-163)
extern "C" int sp_ogm_add_point_cloud(sp_occupancy_grid_map* m, const float* points, const float* covs, const float* rgb,
                                      const float* intensities, size_t n, const float* sensor_pose_host16, void* stream) {
    using namespace sp;
    if (!m || (n && !points)) return SP_ERR_INVALID_ARGUMENT;
    if (n >= (1ull << 32)) { sp_set_error("[OccupancyGridMap] more than 2^32 points"); return SP_ERR_INVALID_ARGUMENT; }
    if (n == 0) return SP_OK;  // :130-132: no rehash, no pruning, no new frame (unlike VoxelHashMap, where an empty cloud is a frame)
    hipStream_t st = as_stream(stream);
    int rc = m->ensure_rehash(st, rehash_launch(m, st));  // :634-641
    if (rc != SP_OK) return rc;
    m->note_attributes(covs, rgb, intensities);
    const float4* pts = reinterpret_cast<const float4*>(points);
    if ((rc = m->write_counter(st, (unsigned)m->voxel_num)) != SP_OK) return rc;
    ogm_hit_kernel<<<stream_grid(n), kBlock, 0, st>>>(m->t, pts, reinterpret_cast<const float4*>(covs),
                                                     reinterpret_cast<const float4*>(rgb), intensities, (unsigned)n,
                                                     pose_arg(sensor_pose_host16), m->voxel_size_inv, m->has_cov, m->has_rgb,
                                                     m->has_intensity, m->frame_index, m->counter);
    if ((rc = m->read_voxel_num(st)) != SP_OK) return rc;
    if (m->free_space_updates && m->log_odds_miss != 0.0f)
        if ((rc = carve(m, pts, (unsigned)n, sensor_pose_host16, st)) != SP_OK) return rc;
    const unsigned cap_blocks = div_up((size_t)m->t.capacity, kBlock);
    ogm_apply_kernel<<<cap_blocks, kBlock, 0, st>>>(m->t, m->log_odds_hit, m->log_odds_miss, m->min_log_odds, m->max_log_odds);
    if ((rc = launch_status()) != SP_OK) return rc;
    if (m->voxel_pruning && m->frame_index >= m->stale_frame_threshold) {  // :1490-1492
        if ((rc = m->write_counter(st, 0)) != SP_OK) return rc;
        ogm_prune_kernel<<<cap_blocks, kBlock, 0, st>>>(m->t, m->frame_index, m->stale_frame_threshold, m->counter);
        if ((rc = m->read_voxel_num(st)) != SP_OK) return rc;
    } else if ((rc = hip_status(hipStreamSynchronize(st))) != SP_OK) {  // the reference waits for the apply kernel (:1482)
        return rc;
    }
    ++m->frame_index;
    return SP_OK;
}

// extract_occupied_points (:169-181) + extract_occupied_points_impl (:1530-1639)
extern "C" int sp_ogm_extract_occupied_points(sp_occupancy_grid_map* m, const float* sensor_xyz_host3, float max_distance,
                                              float* points_out, float* covs_out, float* rgb_out, float* intensities_out,
                                              uint64_t* keys_out_opt, size_t out_capacity, size_t* n_out_host, void* stream) {
    using namespace sp;
    if (!m || !sensor_xyz_host3 || !n_out_host) return SP_ERR_INVALID_ARGUMENT;
    *n_out_host = 0;
    if (m->voxel_num == 0) return SP_OK;
    if (!points_out || out_capacity < m->voxel_num) {
        sp_set_error("[OccupancyGridMap::extract_occupied_points] output arrays must hold sp_ogm_info(SP_OGM_INFO_VOXEL_NUM) entries");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    int rc = flag_and_scan(m, true, sensor_xyz_host3, max_distance, st);
    if (rc != SP_OK) return rc;
    ogm_extract_kernel<<<div_up((size_t)m->t.capacity, kBlock), kBlock, 0, st>>>(
        m->t, m->flags, m->pos, (unsigned)out_capacity, m->mean_rows(points_out, covs_out, rgb_out, intensities_out, keys_out_opt));
    return m->read_total(st, n_out_host);
}

// extract_visible_points (:183-411). Output rows are in table-slot order, as for extract_occupied_points.
extern "C" int sp_ogm_extract_visible_points(sp_occupancy_grid_map* m, const float* sensor_pose_host16, float max_distance,
                                             float horizontal_fov, float vertical_fov, float* points_out, float* covs_out,
                                             float* rgb_out, float* intensities_out, uint64_t* keys_out_opt, size_t out_capacity,
                                             size_t* n_out_host, void* stream) {
    using namespace sp;
    if (!m || !sensor_pose_host16 || !n_out_host) return SP_ERR_INVALID_ARGUMENT;
    *n_out_host = 0;
    bool finite = !std::isnan(max_distance) && std::isfinite(horizontal_fov) && std::isfinite(vertical_fov);  // +inf: no bound
    for (int i = 0; i < 16; ++i)  // the sensor position (12..14) is judged by its cell, below
        if (i < 12 || i == 15) finite = finite && std::isfinite(sensor_pose_host16[i]);
    if (!finite) {  // the reference would compare against NaN limits; refused here, before any HIP call
        sp_set_error("[OccupancyGridMap::extract_visible_points] sensor_pose, max_distance and the fields of view must be finite");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (m->voxel_num == 0) return SP_OK;
    if (!points_out || out_capacity < m->voxel_num) {
        sp_set_error("[OccupancyGridMap::extract_visible_points] output arrays must hold sp_ogm_info(SP_OGM_INFO_VOXEL_NUM) entries");
        return SP_ERR_INVALID_ARGUMENT;
    }
    const float ox = sensor_pose_host16[12], oy = sensor_pose_host16[13], oz = sensor_pose_host16[14];
    const float inv = m->voxel_size_inv, lim = (float)kCellOffset;
    const float fx = std::floor(ox * inv), fy = std::floor(oy * inv), fz = std::floor(oz * inv);
    // a sensor at a non-finite position or outside the 21-bit cell range sees nothing, as a frame from it carves nothing (the
    // reference would walk millions of rejected cells)
    if (!(fx >= -lim && fx < lim && fy >= -lim && fy < lim && fz >= -lim && fz < lim)) return SP_OK;
    constexpr float kFovTolerance = 1e-6f;  // :475-477; kPi is the same float
    horizontal_fov = std::min(std::max(horizontal_fov, kFovTolerance), kPi - kFovTolerance);  // :197-198
    vertical_fov = std::min(std::max(vertical_fov, kFovTolerance), 2.0f * kPi - kFovTolerance);
    Frustum f;
    f.sx = ox; f.sy = oy; f.sz = oz;
    f.max_dist_sq = max_distance * max_distance;
    f.cos_limit_horizontal = std::cos(horizontal_fov * 0.5f);  // :245-248, on the host
    f.cos_limit_vertical = std::cos(vertical_fov * 0.5f);
    f.include_backward = horizontal_fov >= (kPi - kFovTolerance);
    hipStream_t st = as_stream(stream);
    int rc = m->ensure_scratch();
    if (rc != SP_OK) return rc;
    const unsigned cap_blocks = div_up((size_t)m->t.capacity, kBlock);
    ogm_visible_flag_kernel<<<cap_blocks, kBlock, 0, st>>>(m->t, m->occupancy_threshold_log_odds, pose_arg(sensor_pose_host16), f,
                                                          m->flags);
    if ((rc = m->scan_flags(st)) != SP_OK) return rc;
    // Candidates are compacted before the walk: the table is at most 0.7 full and a frustum keeps a few per cent of it, so with one
    // lane per slot most of every wave would idle for as long as its longest ray.
    ogm_candidate_list_kernel<<<cap_blocks, kBlock, 0, st>>>(m->flags, m->pos, m->t.capacity, m->list);
    ogm_visible_walk_kernel<<<stream_grid(m->voxel_num), kBlock, 0, st>>>(m->t, m->list, m->pos + m->t.capacity,
                                                                         m->occupancy_threshold_log_odds, ox, oy, oz, inv,
                                                                         m->voxel_size, m->flags);
    if ((rc = launch_status()) != SP_OK) return rc;
    if ((rc = m->scan_flags(st)) != SP_OK) return rc;
    ogm_extract_kernel<<<cap_blocks, kBlock, 0, st>>>(
        m->t, m->flags, m->pos, (unsigned)out_capacity, m->mean_rows(points_out, covs_out, rgb_out, intensities_out, keys_out_opt));
    return m->read_total(st, n_out_host);
}

extern "C" int sp_ogm_export(sp_occupancy_grid_map* m, uint64_t* keys_out, uint32_t* hit_count_out, uint32_t* miss_count_out,
                             float* log_odds_out, uint32_t* last_updated_out, float* sum_xyz_out, float* cov_sums_out,
                             float* rgb_sums_out, float* intensity_sums_out, size_t out_capacity, size_t* n_out_host, void* stream) {
    using namespace sp;
    if (!m || !n_out_host) return SP_ERR_INVALID_ARGUMENT;
    *n_out_host = 0;
    if (m->voxel_num == 0) return SP_OK;
    if (out_capacity < m->voxel_num) {
        sp_set_error("[OccupancyGridMap::export] output arrays must hold sp_ogm_info(SP_OGM_INFO_VOXEL_NUM) entries");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    int rc = flag_and_scan(m, false, nullptr, 0.0f, st);
    if (rc != SP_OK) return rc;
    ogm_export_kernel<<<div_up((size_t)m->t.capacity, kBlock), kBlock, 0, st>>>(
        m->t, m->flags, m->pos, (unsigned)out_capacity, keys_out, hit_count_out, miss_count_out, log_odds_out, last_updated_out,
        sum_xyz_out, cov_sums_out, rgb_sums_out, intensity_sums_out);
    return m->read_total(st, n_out_host);
}

extern "C" int sp_ogm_overlap_ratio(const sp_occupancy_grid_map* m, const float* points, size_t n, const float* sensor_pose_host16,
                                    float* ratio_out_host, void* stream) {
    if (!m) return SP_ERR_INVALID_ARGUMENT;
    return m->overlap_ratio<sp::kOgmMaxProbe>(sp::Occupied{m->occupancy_threshold_log_odds}, points, n, sensor_pose_host16,
                                              ratio_out_host, sp::as_stream(stream));
}

// voxel_probability (:85-93): compute_key (:569-589) on the host, the probe on the device, the logistic on the host
extern "C" int sp_ogm_voxel_probability(const sp_occupancy_grid_map* m, const float* xyz_host3, float* probability_out_host,
                                        void* stream) {
    using namespace sp;
    if (!m || !xyz_host3 || !probability_out_host) return SP_ERR_INVALID_ARGUMENT;
    *probability_out_host = 0.5f;
    uint64_t key = 0;
    for (int a = 0; a < 3; ++a) {
        const float c = std::floor(xyz_host3[a] * m->voxel_size_inv) + (float)kCellOffset;  // exact: |floor| < 2^24 where it matters
        if (!(c >= 0.0f && c <= (float)kCellMask)) return SP_OK;  // the invalid key is in no slot's live data
        key |= (uint64_t)c << (21 * a);
    }
    hipStream_t st = as_stream(stream);
    ogm_lookup_kernel<<<1, 1, 0, st>>>(m->t, key, m->counter);
    unsigned res[2] = {0, 0};
    int rc = launch_status();
    if (rc == SP_OK) rc = m->read_counter(st, res, 2);
    if (rc != SP_OK || !res[0]) return rc;
    float lo;
    static_assert(sizeof(lo) == sizeof(res[1]), "");
    __builtin_memcpy(&lo, &res[1], sizeof(lo));
    *probability_out_host = 1.0f / (1.0f + std::exp(-lo));  // :563
    return SP_OK;
}
