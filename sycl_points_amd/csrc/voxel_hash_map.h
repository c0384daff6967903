// sp_voxel_hash_map as the two translation units that work on it see it: voxel_hash_map.hip (accumulation, removal, export) and
// voxel_registration.hip (the registration rows and the kernels that align a scan against the map).
#pragma once
#include "sp_voxel_table.h"

namespace sp {
constexpr unsigned kVhmMaxProbe = 100;  // voxel_hash_map.hpp:505
using VhmTable = VoxelTable<float4>;    // core: sum_x, sum_y, sum_z, count (uint32 bits)
}  // namespace sp

struct sp_voxel_hash_map : sp::VoxelMapState<float4> {
    uint32_t max_staleness = 100, remove_old_data_cycle = 10, min_num_point = 1, staleness_counter = 0;
    // Everything that changes what a lookup in the table finds, or what a voxel's row would hold, advances the generation
    // (touch()): add_point_cloud, a rehash, remove_old_data, clear, setting voxel_size or min_num_point.
    uint64_t generation = 1;
    void touch() { ++generation; }
    // The registration rows (sp_vhm_prepare_registration): three float4 per slot, valid for reg_generation / reg_type.
    float4* reg_rows = nullptr;
    size_t reg_rows_cap = 0;
    uint64_t reg_generation = 0;
    int reg_type = -1;
    // The last sp_vhm_linearize: where its frozen slots lie, for how many points, at which generation (sp_vhm_error asks).
    mutable const void* lin_workspace = nullptr;
    mutable size_t lin_n = 0;
    mutable uint64_t lin_generation = 0;
};
