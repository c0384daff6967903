// Registration::align against a VoxelHashMap from MANY initial guesses in one launch (sp_vhm_align_batch): relocalisation against
// the one target that persists across frames — start-up without a pose, a yaw sweep after tracking is lost, a loop-closure check
// against an old submap. The host-driven loop of voxel_registration.hip costs two launches and a read-back per linearisation and
// per LM / dog-leg trial, 20 to 60 round trips an alignment, times the number of guesses.
//
// vhm_optimize_batch_kernel is gicp_optimize_batch_kernel's launch shape (registration_batch.hip) around the voxel per-point
// bodies (sp_voxel_registration.h): a plain grid of `batch` workgroups, workgroup b runs the WHOLE alignment of hypothesis b. A
// step is a pass of the workgroup's lanes over the source (vhm_linearize_point to linearise: every point is looked up again,
// there is nothing to reuse; vhm_error_point over the frozen slots for a trial), the step's totals are summed in LDS
// (block_reduce_lds) and one lane runs the optimiser's state machine (sp_optimizer.h) on LDS. Hypotheses share nothing they
// write: the map's keys and rows and the packed source rows are read-only, the frozen slots of hypothesis b are its own uint32
// array in the caller's workspace. So no workgroup ever waits for another: no counter, no residency requirement, no bounded
// wait, any batch on any stream (a capturing one included). Every loop is bounded: max_iterations, lm_max_inner_iterations,
// SP_OPT_MAX_LEVELS, kVhmMaxProbe. The map is only read; its generation and sp_vhm_linearize's bookkeeping stay as they are.
#include "sp_voxel_registration.h"
#include "sp_optimizer.h"

namespace sp {
namespace {

struct VhmBatchArgs {
    unsigned* slots;       // batch x slot_stride: the hypotheses' frozen correspondences
    size_t slot_stride;
    uint64_t* corr_keys;   // optional: batch x n
    const float* T_init;   // device: batch x 16, column-major
    float* T_out;          // device: batch x 16 (may alias T_init: workgroup b reads its pose before it writes anything)
    sp_opt_params opt;
    float scales[SP_OPT_MAX_LEVELS];
    int n_levels;
    sp_align_result* results;
};

// The step's totals (block_reduce_lds: sums | uint32 count) into the state machine. Every linearisation looks every point up.
__device__ __forceinline__ void vhm_after_linearize(OptState& S, const float* tot, unsigned n) {
    unpack_totals(tot, kAcc - 1, &S.slin);
    ++S.ctl.n_lin;
    S.ctl.searched += n;
    opt_after_linearize(S, true);
}
__device__ __forceinline__ void vhm_after_trial(OptState& S, const float* tot) {
    opt_after_trial(S, tot[0], __float_as_uint(tot[1]), true);
}
// (Inlined at every workgroup size: this unit is built with every device function inlined. A real function — the state machine
// as gicp_optimize_batch_kernel calls it at 1024 lanes, or gn_update_impl as the compiler leaves it on its own — saves the
// registers it must preserve on the stack: 8 to 232 bytes of scratch per lane for a kernel that otherwise needs none.)

template <int LOSS, bool P2D, int NV, int BLOCK>
__global__ __launch_bounds__(BLOCK) void vhm_optimize_batch_kernel(VhmRegArgs R, VhmBatchArgs A) {
    __shared__ OptState S;
    __shared__ float tot[kPartial];
    const size_t b = blockIdx.x;
    sp_align_result* const result = A.results + b;
    R.slots = A.slots + b * A.slot_stride;
    if (A.corr_keys) R.corr_keys = A.corr_keys + b * (size_t)R.n;
    if (threadIdx.x < 16) {
        const float v = A.T_init[b * 16 + threadIdx.x];
        S.sT[threadIdx.x] = v;
        S.sTlin[threadIdx.x] = v;
    } else if (threadIdx.x == 32) {
        OptCtl c;
        opt_start(c, A.opt, 0);
        S.ctl = c;
        S.opt = A.opt;
        S.n_levels = A.n_levels;
        S.reuse = 0;  // no correspondence survives a linearisation
        S.result = result;
    } else if (threadIdx.x >= 64 && threadIdx.x < 64 + 48) {
        reinterpret_cast<float*>(&S.slin)[threadIdx.x - 64] = 0.0f;
    }
    __syncthreads();
    for (;;) {
        const int phase = S.ctl.phase;  // uniform over the workgroup
        R.scale = A.scales[S.ctl.level];
        if (phase == PHASE_LIN) {
            const Rigid T = uniform_pose(S.sT);
            float acc[kAcc - 1];
            unsigned cnt = 0;
#pragma unroll
            for (int e = 0; e < kAcc - 1; ++e) acc[e] = 0.0f;
            for (unsigned i = threadIdx.x; i < R.n; i += BLOCK) vhm_linearize_point<LOSS, P2D, NV>(R, T, i, acc, cnt);
            block_reduce_lds<kAcc - 1, BLOCK>(acc, cnt, 0u, tot);
        } else {  // PHASE_TRIAL: the lane that looked a point up also evaluates it
            const Rigid T = uniform_pose(S.sTt);
            float acc[1] = {0.0f};
            unsigned cnt = 0;
            for (unsigned i = threadIdx.x; i < R.n; i += BLOCK) vhm_error_point<LOSS, P2D>(R, T, i, acc, cnt);
            block_reduce_lds<1, BLOCK>(acc, cnt, 0u, tot);
        }
        if (threadIdx.x == 0) {
            if (phase == PHASE_LIN) vhm_after_linearize(S, tot, R.n);
            else vhm_after_trial(S, tot);
        }
        __syncthreads();
        if (S.ctl.done) break;
    }
    // the result block as sp_gicp_align_batch writes it: the done flag goes last, behind a system-scope release
    const unsigned t = threadIdx.x;
    if (t < 16) { result->T[t] = S.sT[t]; A.T_out[b * 16 + t] = S.sT[t]; }
    else if (t < 32) result->T_lin[t - 16] = S.sTlin[t - 16];
    else if (t >= 64 && t < 100) result->H[t - 64] = S.slin.H[t - 64];
    else if (t >= 128 && t < 134) result->b[t - 128] = S.slin.b[t - 128];
    else if (t == 192) opt_result_scalars(S, result);
    __syncthreads();
    if (t == 0) {
        __threadfence_system();
        __hip_atomic_store(&result->pad[0], (unsigned)SP_ALIGN_RESULT_DONE, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
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
    if (n_levels < 1 || n_levels > SP_OPT_MAX_LEVELS) return invalid("[sp_vhm_align_batch] n_levels must be in 1..SP_OPT_MAX_LEVELS");
    if (opt->method != SP_OPT_GAUSS_NEWTON && opt->method != SP_OPT_LEVENBERG_MARQUARDT && opt->method != SP_OPT_POWELL_DOGLEG)
        return invalid("[sp_vhm_align_batch] unknown optimization method");
    if (opt->max_iterations < 1 || opt->max_iterations > 65535)
        return invalid("[sp_vhm_align_batch] max_iterations must be in 1..65535 (0 iterations: the results are the initial guesses)");
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
    for (int l = 0; l < SP_OPT_MAX_LEVELS; ++l) A.scales[l] = robust_scales[l < n_levels ? l : n_levels - 1];
    A.n_levels = n_levels;
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
