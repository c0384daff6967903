// CPU restatement of OccupancyGridMap::extract_visible_points (algorithms/mapping/occupancy_grid_map.hpp:183-411 of the reference) as
// this project specifies it: single-threaded, a function of an exported state (the arrays of sp_ogm_export /
// ogm_restate_export) and the call's arguments alone. Voxels are looked up by key in a map of its own, not in a hash-table layout.
// Compiled by the tests that use it with -O2 -ffp-contract=off; every fused multiply-add is an explicit std::fma.
//
// Where it departs from the reference it does so with the device, on purpose:
//   * the walk from the sensor to a candidate's centroid is the BOUNDED walk of occupancy_grid_restate.cpp (bounded_walk): exactly
//     |dix| + |diy| + |diz| steps, the last one, into the candidate's own cell, not tested;
//   * the two cosines of the frustum test are forward / sqrt(norm_sq), both correctly rounded (the reference: forward * rsqrt);
//   * the visible voxels come out in the order of the input rows (the export's: table-slot order);
//   * a sensor position that is non-finite or whose cell lies outside the 21-bit range sees nothing.
#include <algorithm>
#include <unordered_map>

#include "occupancy_grid_restate.cpp"

namespace {

constexpr float kPi = 3.1415927f, kFovTolerance = 1e-6f, kOcclusionEpsilon = 1e-6f;  // :475-477

struct Voxel { float cx, cy, cz; bool occupied; };

float chain3(float a0, float b0, float a1, float b1, float a2, float b2) {  // eigen_utils::multiply<3, 3>'s row (eigen_utils.hpp:114)
    return std::fma(a2, b2, std::fma(a1, b1, std::fma(a0, b0, 0.0f)));
}
float clamp_unit(float c) { return c < -1.0f ? -1.0f : (c > 1.0f ? 1.0f : c); }

}  // namespace

extern "C" {

// visible_keys_out holds n entries. counts_out[0] = candidates, [1] = occluded candidates, [2] = the longest walk begun (steps).
// Returns the number of visible voxels.
uint64_t ogm_visible_restate(const uint64_t* keys, const uint32_t* hit_count, const float* log_odds, const float* sum_xyz, uint64_t n,
                             float voxel_size, float threshold_log_odds, const float* pose16, float max_distance,
                             float horizontal_fov, float vertical_fov, uint64_t* visible_keys_out, uint64_t* counts_out) {
    counts_out[0] = counts_out[1] = counts_out[2] = 0;
    const float inv = 1.0f / voxel_size;
    const float ox = pose16[12], oy = pose16[13], oz = pose16[14];
    const float fx = std::floor(ox * inv), fy = std::floor(oy * inv), fz = std::floor(oz * inv);
    const float lim = (float)kOffset;
    if (!(fx >= -lim && fx < lim && fy >= -lim && fy < lim && fz >= -lim && fz < lim)) return 0;

    horizontal_fov = std::clamp(horizontal_fov, kFovTolerance, kPi - kFovTolerance);  // :197-198
    vertical_fov = std::clamp(vertical_fov, kFovTolerance, 2.0f * kPi - kFovTolerance);
    const float max_dist_sq = max_distance * max_distance;  // :244-248
    const float cos_limit_horizontal = std::cos(horizontal_fov * 0.5f), cos_limit_vertical = std::cos(vertical_fov * 0.5f);
    const bool include_backward = horizontal_fov >= (kPi - kFovTolerance);

    std::unordered_map<uint64_t, Voxel> voxels;
    voxels.reserve((size_t)n);
    for (uint64_t i = 0; i < n; ++i) {
        if (keys[i] == kInvalid || keys[i] == kDeleted) continue;
        const float inv_count = 1.0f / (float)hit_count[i];
        voxels[keys[i]] = Voxel{sum_xyz[3 * i] * inv_count, sum_xyz[3 * i + 1] * inv_count, sum_xyz[3 * i + 2] * inv_count,
                                hit_count[i] > 0u && !(log_odds[i] < threshold_log_odds)};
    }

    uint64_t visible = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const auto it = voxels.find(keys[i]);
        if (it == voxels.end() || !it->second.occupied) continue;  // :252-260
        const Voxel& v = it->second;
        const float dx = v.cx - ox, dy = v.cy - oy, dz = v.cz - oz;  // :262-273
        const float dist_sq = dx * dx + dy * dy + dz * dz;
        if (!(dist_sq <= max_dist_sq)) continue;
        // R^T d (:274-276): the rotation block of sensor_pose.inverse() is the transpose, element (i, j) = pose16[4 * i + j]
        const float lx = chain3(pose16[0], dx, pose16[1], dy, pose16[2], dz);
        const float ly = chain3(pose16[4], dx, pose16[5], dy, pose16[6], dz);
        const float lz = chain3(pose16[8], dx, pose16[9], dy, pose16[10], dz);
        if (!include_backward && lx <= 0.0f) continue;  // :278-311
        const float forward = include_backward ? std::fabs(lx) : lx;
        const float h_sq = forward * forward + ly * ly, v_sq = forward * forward + lz * lz;
        const float cos_h = h_sq > 0.0f ? clamp_unit(forward / std::sqrt(h_sq)) : 1.0f;
        if (cos_h < cos_limit_horizontal) continue;
        const float cos_v = v_sq > 0.0f ? clamp_unit(forward / std::sqrt(v_sq)) : 1.0f;
        if (cos_v < cos_limit_vertical) continue;
        ++counts_out[0];

        bool occluded = false;
        const float w[4] = {v.cx, v.cy, v.cz, 1.0f};
        if (std::sqrt(dist_sq) > voxel_size && oracle::compute_voxel_bit(w, inv) != kInvalid) {  // :313-357
            const int tx = (int)std::floor(v.cx * inv), ty = (int)std::floor(v.cy * inv), tz = (int)std::floor(v.cz * inv);
            const uint64_t steps = bounded_walk(ox, oy, oz, v.cx, v.cy, v.cz, inv, [&](int x, int y, int z) {
                if (occluded || (x == tx && y == ty && z == tz)) return;  // past the first occluder | the last step, by construction
                const uint64_t k = cell_key(x, y, z);
                if (k == kInvalid || k == keys[i]) return;
                const auto o = voxels.find(k);
                if (o == voxels.end() || !o->second.occupied) return;
                const float ex = o->second.cx - ox, ey = o->second.cy - oy, ez = o->second.cz - oz;
                if (ex * ex + ey * ey + ez * ez + kOcclusionEpsilon < dist_sq) occluded = true;
            });
            counts_out[2] = std::max(counts_out[2], steps);
        }
        if (occluded) { ++counts_out[1]; continue; }
        visible_keys_out[visible++] = keys[i];
    }
    return visible;
}

}  // extern "C"
