// Registration::align against a VoxelHashMap from MANY initial guesses in one launch (sp_vhm_align_batch): relocalisation against
// the one target that persists across frames — start-up without a pose, a yaw sweep after tracking is lost, a loop-closure check
// against an old submap. The host-driven loop of voxel_registration.hip costs two launches and a read-back per linearisation and
// per LM / dog-leg trial, 20 to 60 round trips an alignment, times the number of guesses.
//
// vhm_optimize_batch_kernel is the one-workgroup-per-guess shell of sp_optimize_batch.h (the launch shape and why no workgroup
// ever waits for another are explained there) around the voxel per-point bodies (sp_voxel_registration.h): vhm_linearize_point to
// linearise (every point is looked up again, there is nothing to reuse; bounded by kVhmMaxProbe), vhm_error_point over the frozen
// slots for a trial. What a hypothesis owns is its uint32 array of frozen slots in the caller's workspace (and its row of
// corr_keys, when asked for); the map's keys and rows and the packed source rows are read-only. The map is only read; its
// generation and sp_vhm_linearize's bookkeeping stay as they are.
#include "sp_voxel_registration.h"
#include "sp_optimize_batch.h"

namespace sp {
namespace {

struct VhmBatchArgs : BatchCommon {  // (reuse = 0: no correspondence survives a linearisation)
    unsigned* slots;       // batch x slot_stride: the hypotheses' frozen correspondences
    size_t slot_stride;
    uint64_t* corr_keys;   // optional: batch x n
};

template <int LOSS, bool P2D, int NV>
struct VhmBatchProblem {
    VhmRegArgs& R;
    const VhmBatchArgs& A;
    __device__ __forceinline__ unsigned n() const { return R.n; }
    __device__ __forceinline__ void hypothesis(size_t b) {
        R.slots = A.slots + b * A.slot_stride;
        if (A.corr_keys) R.corr_keys = A.corr_keys + b * (size_t)R.n;
    }
    __device__ __forceinline__ void scale(float s) { R.scale = s; }
    __device__ __forceinline__ void cache_valid(int) {}
    __device__ __forceinline__ void linearize(const Rigid& T, unsigned i, float (&acc)[kAcc - 1], unsigned& cnt, unsigned&) {
        vhm_linearize_point<LOSS, P2D, NV>(R, T, i, acc, cnt);
    }
    __device__ __forceinline__ void error(const Rigid& T, const Rigid&, unsigned i, float (&acc)[1], unsigned& cnt) {
        vhm_error_point<LOSS, P2D>(R, T, i, acc, cnt);
    }
    __device__ __forceinline__ unsigned searched(const float*) const { return R.n; }  // every linearisation looks every point up
};

// The state machine is inlined at every workgroup size (CALLS = false), and this unit is built with every device function
// inlined. A real function — the state machine as gicp_optimize_batch_kernel calls it at 1024 lanes, or gn_update_impl as the
// compiler leaves it on its own — saves the registers it must preserve on the stack: 8 to 232 bytes of scratch per lane for a
// kernel that otherwise needs none.
template <int LOSS, bool P2D, int NV, int BLOCK>
__global__ __launch_bounds__(BLOCK) void vhm_optimize_batch_kernel(VhmRegArgs R, VhmBatchArgs A) {
    VhmBatchProblem<LOSS, P2D, NV> Q{R, A};
    optimize_batch_workgroup<BLOCK, false>(Q, A);
}

// Lanes per workgroup once the source has more than 256 points: the largest of 1024 / 512 / 256 at which every instantiation of
// that NV shows ScratchSize 0 in lib/voxel_registration_batch.resources.txt (DESIGN 4.19 has the table). 512 and 256 lanes leave
// a lane 256 registers: 139-154 are used with 1 and 7 probed cells, 219-235 with 27. The 128 registers of a 1024-lane workgroup
// are too few for every NV: 21 to 30 spilled registers with 1 and 7 cells, 139 with 27.
template <int NV>
constexpr int kVhmBatchBlock = NV == 1 ? 512    // 1024: 21 spilled registers, 84 bytes of scratch
                                : NV == 7 ? 512  // 1024: 30 spilled registers, 84 bytes of scratch
                                          : 512; // 1024: 139 spilled registers, 384 bytes of scratch

// The workspace: two float4 per source point (GICP's packed source rows) | batch arrays of slots, each 16-byte aligned
size_t vhm_batch_slot_stride(size_t n) { return (n + 3) / 4 * 4; }
size_t vhm_batch_bytes(size_t n, size_t batch) {
    if (n == 0 || n > (size_t)SP_VHM_ALIGN_BATCH_MAX_POINTS || batch == 0 || batch > (size_t)SP_ALIGN_BATCH_MAX) return 0;
    return n * 2 * sizeof(float4) + batch * vhm_batch_slot_stride(n) * sizeof(unsigned);
}

}  // namespace
}  // namespace sp

extern "C" size_t sp_vhm_align_batch_workspace_bytes(size_t n, size_t batch) { return sp::vhm_batch_bytes(n, batch); }

extern "C" int sp_vhm_align_batch(const sp_voxel_hash_map* m, const float* src_points, const float* src_covs, size_t n,
                                  const float* T_init_device, float* T_out_device, size_t batch, const sp_factor_params* params,
                                  const sp_opt_params* opt, const float* robust_scales, int n_levels, int neighbor_voxels,
                                  sp_align_result* results_device, uint64_t* corr_keys_out_opt, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    using namespace sp;
    if (!m || !src_points || !params || !opt || !T_init_device || !T_out_device || !results_device || !robust_scales)
        return invalid("[sp_vhm_align_batch] null argument");
    if (const int rc = check_opt_args("sp_vhm_align_batch", opt, n_levels, "the results are the initial guesses"); rc != SP_OK) return rc;
    if (const int rc = check_reg_type(params->reg_type); rc != SP_OK) return rc;
    if (params->rotation_constraint_enable) return invalid("[VoxelHashMap registration] the rotation constraint is not supported");
    if (!m->has_cov) return invalid("[VoxelHashMap registration] the map holds no covariances");
    if (!rows_ready(m, params->reg_type))
        return invalid("[sp_vhm_align_batch] the registration rows are not those of the map as it is now and of this reg_type: "
                       "call sp_vhm_prepare_registration");
    if (neighbor_voxels != 1 && neighbor_voxels != 7 && neighbor_voxels != 27)
        return invalid("[VoxelHashMap registration] neighbor_voxels must be 1, 7 or 27");
    if (n == 0 || n > (size_t)SP_VHM_ALIGN_BATCH_MAX_POINTS)
        return invalid("[sp_vhm_align_batch] the source must hold 1..SP_VHM_ALIGN_BATCH_MAX_POINTS points");
    if (batch == 0 || batch > (size_t)SP_ALIGN_BATCH_MAX) return invalid("[sp_vhm_align_batch] batch must be in 1..SP_ALIGN_BATCH_MAX");
    const bool p2d = params->reg_type == SP_REG_POINT_TO_DISTRIBUTION;
    if (!p2d && !src_covs) {
        sp_set_error("[Registration::validate_params] Covariance matrices of source and target must be pre-computed before "
                     "performing GICP matching.");
        return SP_ERR_RUNTIME;
    }
    if (!workspace || workspace_bytes < vhm_batch_bytes(n, batch))
        return invalid("[sp_vhm_align_batch] workspace too small (sp_vhm_align_batch_workspace_bytes)");
    if (params->robust_type < SP_LOSS_NONE || params->robust_type > SP_LOSS_GEMAN_MCCLURE) return unknown_combination();  // (before anything is enqueued)
    hipStream_t st = as_stream(stream);
    float4* const src_rows = static_cast<float4*>(workspace);
    if (!p2d) {
        vhm_source_rows_kernel<<<div_up(n, kBlock), kBlock, 0, st>>>(reinterpret_cast<const float4*>(src_covs), (unsigned)n, src_rows);
        if (const int rc = launch_status(); rc != SP_OK) return rc;
    }
    VhmRegArgs R;
    R.keys = m->t.key;
    R.rows = m->reg_rows;
    R.capacity = m->t.capacity;
    R.src = reinterpret_cast<const float4*>(src_points);
    R.src_rows = src_rows;
    R.slots = nullptr;
    R.corr_keys = nullptr;
    R.n = (unsigned)n;
    R.inv = m->voxel_size_inv;
    R.max_d2 = params->max_correspondence_distance * params->max_correspondence_distance;
    R.scale = params->robust_scale;
    R.pose = query_pose(nullptr, 0);
    VhmBatchArgs A;
    A.slots = reinterpret_cast<unsigned*>(src_rows + 2 * n);
    A.slot_stride = vhm_batch_slot_stride(n);
    A.corr_keys = corr_keys_out_opt;
    A.T_init = T_init_device;
    A.T_out = T_out_device;
    A.opt = *opt;
    fill_level_scales(A.scales, robust_scales, n_levels);
    A.n_levels = n_levels;
    A.reuse = 0;
    A.results = results_device;
    const unsigned grid = (unsigned)batch;
    const int rc = with_loss(params->robust_type, [&](auto L) {
        return with_bool<false>(p2d, [&](auto P2D) {
            constexpr int loss = decltype(L)::value;
            constexpr bool p = decltype(P2D)::value;
            auto launch = [&](auto NVc) {
                constexpr int NV = decltype(NVc)::value;
                if (n <= 256) vhm_optimize_batch_kernel<loss, p, NV, 256><<<grid, 256, 0, st>>>(R, A);
                else vhm_optimize_batch_kernel<loss, p, NV, kVhmBatchBlock<NV>><<<grid, kVhmBatchBlock<NV>, 0, st>>>(R, A);
            };
            if (neighbor_voxels == 1) launch(std::integral_constant<int, 1>{});
            else if (neighbor_voxels == 7) launch(std::integral_constant<int, 7>{});
            else launch(std::integral_constant<int, 27>{});
            return SP_OK;
        });
    });
    if (rc != SP_OK) return rc;
    return launch_status();
}
