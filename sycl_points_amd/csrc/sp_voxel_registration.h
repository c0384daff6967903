// The per-point bodies of voxelised GICP: what one lane does with one source point against a VoxelHashMap's
// registration rows. vhm_linearize_point is the correspondence search by hash lookup plus the linearisation, vhm_error_point the
// factor's error over a frozen slot. Called by the grid-stride kernels of voxel_registration.hip (one launch per step, a
// host-driven optimiser) and by the one-workgroup-per-hypothesis kernel of voxel_registration_batch.hip: one body, the same bits.
#ifndef SP_VOXEL_REGISTRATION_H
#define SP_VOXEL_REGISTRATION_H

#include "voxel_hash_map.h"
#include "sp_optimizer.h"
#include "sp_cov_normal.h"

namespace sp {
namespace {

constexpr unsigned kNoFrozenSlot = 0xFFFFFFFFu;

// The probing order: the point's own cell, the six face neighbours, the twelve edge neighbours, the eight corner neighbours.
// The first 1 / 7 / 27 entries are the three modes.
struct CellOffsets {
    int8_t d[27][3];
};
constexpr CellOffsets make_cell_offsets() {
    CellOffsets o{};
    int k = 0;
    for (int nz = 0; nz <= 3; ++nz)
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                    if ((dx != 0) + (dy != 0) + (dz != 0) == nz) {
                        o.d[k][0] = (int8_t)dx; o.d[k][1] = (int8_t)dy; o.d[k][2] = (int8_t)dz;
                        ++k;
                    }
    return o;
}
constexpr CellOffsets kCellOffsets = make_cell_offsets();

constexpr int64_t kCellMask = (1 << 21) - 1;
constexpr int64_t kCellOffset = 1 << 20;

// voxel_key3 in two steps: the offset cell coordinates of a finite point (the same arithmetic), then the key of a cell
// next to it, kInvalidKey when that cell lies outside the 21 bits of an axis.
__device__ __forceinline__ uint64_t cell_key(int64_t c0, int64_t c1, int64_t c2) {
    if (c0 < 0 || kCellMask < c0 || c1 < 0 || kCellMask < c1 || c2 < 0 || kCellMask < c2) return kInvalidKey;
    return ((uint64_t)(c0 & kCellMask)) | ((uint64_t)(c1 & kCellMask) << 21) | ((uint64_t)(c2 & kCellMask) << 42);
}

__device__ __forceinline__ float4 pack_sym_lo(const Mat3& P) {
    return make_float4(P.m[0][0], (P.m[0][1] + P.m[1][0]) * 0.5f, (P.m[0][2] + P.m[2][0]) * 0.5f, P.m[1][1]);
}
__device__ __forceinline__ float4 pack_sym_hi(const Mat3& P) {
    return make_float4((P.m[1][2] + P.m[2][1]) * 0.5f, P.m[2][2], 0.0f, 0.0f);
}

// The packed regularised source covariances of an alignment (GICP): two float4 per source point.
__global__ __launch_bounds__(kBlock) void vhm_source_rows_kernel(const float4* __restrict__ covs, unsigned n, float4* __restrict__ rows) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const Mat3 P = plane_regularize(load_cov(covs + 4 * (size_t)i));
    rows[2 * (size_t)i] = pack_sym_lo(P);
    rows[2 * (size_t)i + 1] = pack_sym_hi(P);
}

inline int check_reg_type(int reg_type) {
    if (reg_type == SP_REG_GICP || reg_type == SP_REG_POINT_TO_DISTRIBUTION) return SP_OK;
    return invalid("[VoxelHashMap registration] reg_type must be GICP or POINT_TO_DISTRIBUTION");
}
inline bool rows_ready(const sp_voxel_hash_map* m, int reg_type) {
    return m->reg_rows != nullptr && m->reg_rows_cap >= (size_t)m->t.capacity && m->reg_generation == m->generation &&
           m->reg_type == reg_type;
}

struct VhmRegArgs {
    const uint64_t* keys;
    const float4* rows;     // three per slot
    unsigned long long capacity;
    const float4* src;      // source points, rows of four floats
    const float4* src_rows; // two per source point (GICP), in the workspace
    unsigned* slots;        // the frozen correspondence of every source point
    uint64_t* corr_keys;    // optional
    unsigned n;
    float inv, max_d2, scale;
    QueryPose pose;
};

// Source point i at pose T (sp_voxel_linearize_body.h: the statements vhm_linearize_kernel has in place), as a function.
template <int LOSS, bool P2D, int NV>
__device__ __forceinline__ void vhm_linearize_point(const VhmRegArgs& A, const Rigid& T, unsigned i, float (&acc)[kAcc - 1],
                                                    unsigned& cnt) {
#define VHM_POINT_DONE return
#include "sp_voxel_linearize_body.h"
#undef VHM_POINT_DONE
}

// The factor's error of source point i at the trial pose T over the slot frozen in A.slots[i]: one row gather per inlier.
template <int LOSS, bool P2D>
__device__ __forceinline__ void vhm_error_point(const VhmRegArgs& A, const Rigid& T, unsigned i, float (&acc)[1], unsigned& cnt) {
    const unsigned s = A.slots[i];
    if (s >= A.capacity) return;  // kNoFrozenSlot, and nothing outside the table is ever read
    const float4 p = A.src[i];
    const float4 m = A.rows[3 * (size_t)s];
    const Sym3 Ct = load_sym(A.rows + 3 * (size_t)s + 1);
    Sym3 Cs{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (!P2D) Cs = load_sym(A.src_rows + 2 * (size_t)i);
    float qx, qy, qz;
    transform_point(T, p.x, p.y, p.z, qx, qy, qz);
    float t[1];
    linearize_terms<LOSS, P2D, true, 1>(T, p.x, p.y, p.z, qx, qy, qz, m.x, m.y, m.z, Cs, Ct, A.scale, t);
    acc[0] += t[0];
    ++cnt;
}

}  // namespace
}  // namespace sp
#endif
