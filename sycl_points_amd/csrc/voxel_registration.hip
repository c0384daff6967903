// Voxelised GICP for gfx950: a scan aligned against a VoxelHashMap itself (sp_vhm_prepare_registration, sp_vhm_prepare_source,
// sp_vhm_linearize, sp_vhm_error; include/sycl_points_amd.h). The reference has no such path: its Submap exports the voxel means,
// builds a KD-tree on them, estimates covariances and searches a neighbour per source point per iteration.
//
// The target of a source point is the Gaussian its voxel already holds in HBM (sp_voxel_table.h: a mean and a log-Euclidean
// covariance mean), and the correspondence search is voxel_table_overlap_kernel's: transform, key, probe. What this file adds:
//   * the registration rows, three float4 per table slot, indexed by the slot itself: (mean, w) | the packed symmetric 3x3 of
//     prepare_cov_kernel (registration.hip) — V diag(1e-3, 1, 1) V^T of the decoded covariance for GICP, its inverse for
//     point-to-distribution. One launch per map generation, one lane per slot, an empty slot costs its key load;
//   * the linearisation: one lane per source point, grid stride. The chain per point is key -> row, two dependent random loads
//     (MI355X_MICROARCH.md "Indexed rows", "Infinity Cache": a 1 M-voxel map is 8 MB of keys and 48 MB of rows, resident on the
//     die between iterations). With 7 or 27 probed cells all first-probe key loads are issued before any is compared; the mean
//     row is read for every hit, the two covariance rows for the winner alone. Bytes per correspondence: 16 (point) + 32 (source
//     rows, GICP) + 8 per probed cell + 16 per hit + 32 for the winner + 4 (+ 8) written;
//   * the trial error over the slots the linearisation froze (the contract of sp_gicp_error_prepared).
// The per-point algebra is sp_linearize.h's (this unit is compiled with -fno-slp-vectorize like its other users), the sums are
// block_reduce_store and reduce_rows_1024 (registration_device.h): a fixed tree, no float atomics, the same bits run after run.
#include "sp_voxel_registration.h"

namespace sp {
namespace {

// The rows of every used slot. The mean is write_mean_row's, the covariance decode_cov's: what downsampling() exports.
template <bool P2D>
__global__ __launch_bounds__(kBlock) void vhm_registration_rows_kernel(VhmTable t, uint32_t min_num_point, float4* __restrict__ rows) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= t.capacity) return;
    if (t.key[i] == kInvalidKey) return;
    const float4 c = t.core[i];
    const unsigned count = __float_as_uint(c.w);
    float4* const row = rows + 3 * (size_t)i;
    if (!(count >= min_num_point && count != 0u)) {
        row[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float inv = 1.0f / (float)count;
    float4 c4[4];
    decode_cov(t.cov[i], inv, c4);
    const Mat3 C = cov_of_columns(c4[0], c4[1], c4[2]);
    const Mat3 P = P2D ? inverse(C) : plane_regularize(C);
    row[0] = make_float4(c.x * inv, c.y * inv, c.z * inv, 1.0f);
    row[1] = pack_sym_lo(P);
    row[2] = pack_sym_hi(P);
}

// (the point's statements in place, not through vhm_linearize_point: sp_voxel_linearize_body.h says why)
template <int LOSS, bool P2D, int NV>
__global__ __launch_bounds__(kBlock) void vhm_linearize_kernel(VhmRegArgs A, float* __restrict__ partials) {
    const Rigid T = load_pose(A.pose);
    float acc[kAcc - 1];
#pragma unroll
    for (int e = 0; e < kAcc - 1; ++e) acc[e] = 0.0f;
    unsigned cnt = 0;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < A.n; i += gridDim.x * kBlock) {
#define VHM_POINT_DONE continue
#include "sp_voxel_linearize_body.h"
#undef VHM_POINT_DONE
    }
    block_reduce_store<kAcc - 1>(acc, cnt, partials + (size_t)blockIdx.x * kPartial);
}

// The factor's error at a trial pose over the frozen slots: one coalesced stream over the source and one row gather per inlier.
template <int LOSS, bool P2D>
__global__ __launch_bounds__(kBlock) void vhm_error_kernel(VhmRegArgs A, float* __restrict__ partials) {
    const Rigid T = load_pose(A.pose);
    float acc[1] = {0.0f};
    unsigned cnt = 0;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < A.n; i += gridDim.x * kBlock) vhm_error_point<LOSS, P2D>(A, T, i, acc, cnt);
    block_reduce_store<1>(acc, cnt, partials + (size_t)blockIdx.x * kPartial);
}

// final_reduce_kernel of registration.hip without its Gauss-Newton step: the same fixed tree over the partial rows
__global__ __launch_bounds__(kFinalThreads) void vhm_final_reduce_kernel(const float* __restrict__ partials, unsigned nblocks, int nv,
                                                                         sp_linearized* __restrict__ out) {
    __shared__ float red[kFinalThreads / 32][kPartial];
    reduce_rows_1024(partials, nblocks, nv, red);
    if (threadIdx.x == 0) unpack_totals(red[0], nv, out);
}

// The workspace: partial rows | slots | source rows, each part 16-byte aligned
constexpr size_t kVhmPartialBytes = (size_t)kMaxBlocks * kPartial * sizeof(float);
size_t slots_bytes(size_t n) { return (n * sizeof(unsigned) + 15) / 16 * 16; }
size_t vhm_workspace_bytes(size_t n) { return kVhmPartialBytes + slots_bytes(n) + n * 2 * sizeof(float4); }
unsigned* ws_slots(void* ws) { return reinterpret_cast<unsigned*>(static_cast<char*>(ws) + kVhmPartialBytes); }
float4* ws_source_rows(void* ws, size_t n) { return reinterpret_cast<float4*>(static_cast<char*>(ws) + kVhmPartialBytes + slots_bytes(n)); }

unsigned vhm_reduce_grid(size_t n) {
    unsigned g = div_up(n, kBlock);
    if (g > (unsigned)kMaxBlocks) g = kMaxBlocks;
    return g ? g : 1;
}

// what sp_vhm_linearize and sp_vhm_error check alike, in this order
int check_call(const char* not_ready, const sp_voxel_hash_map* m, const float* src, size_t n, const sp_factor_params* fp,
               const sp_linearized* out) {
    if (!m || !fp || !out || (n && !src)) return SP_ERR_INVALID_ARGUMENT;
    if (const int rc = check_reg_type(fp->reg_type); rc != SP_OK) return rc;
    if (fp->rotation_constraint_enable) return invalid("[VoxelHashMap registration] the rotation constraint is not supported");
    if (!m->has_cov) return invalid("[VoxelHashMap registration] the map holds no covariances");
    if (!rows_ready(m, fp->reg_type)) return invalid(not_ready);
    if (n >= (1ull << 32)) return invalid("[VoxelHashMap registration] more than 2^32 source points");
    return SP_OK;
}
int check_vhm_workspace(const void* ws, size_t bytes, size_t n) {
    if (!ws || bytes < vhm_workspace_bytes(n))
        return invalid("[VoxelHashMap registration] workspace too small (sp_vhm_registration_workspace_bytes)");
    return SP_OK;
}
VhmRegArgs make_args(const sp_voxel_hash_map* m, const float* src, size_t n, const float* T, int T_dev, const sp_factor_params* fp,
                     void* ws, uint64_t* corr_keys) {
    VhmRegArgs A;
    A.keys = m->t.key;
    A.rows = m->reg_rows;
    A.capacity = m->t.capacity;
    A.src = reinterpret_cast<const float4*>(src);
    A.src_rows = ws_source_rows(ws, n);
    A.slots = ws_slots(ws);
    A.corr_keys = corr_keys;
    A.n = (unsigned)n;
    A.inv = m->voxel_size_inv;
    A.max_d2 = fp->max_correspondence_distance * fp->max_correspondence_distance;
    A.scale = fp->robust_scale;
    A.pose = query_pose(T, T_dev);
    return A;
}

}  // namespace
}  // namespace sp

extern "C" int sp_vhm_prepare_registration(sp_voxel_hash_map* m, int reg_type, void* stream) {
    using namespace sp;
    if (!m) return SP_ERR_INVALID_ARGUMENT;
    if (const int rc = check_reg_type(reg_type); rc != SP_OK) return rc;
    if (!m->has_cov) return invalid("[VoxelHashMap registration] the map holds no covariances");
    hipStream_t st = as_stream(stream);
    const size_t cap = (size_t)m->t.capacity;
    if (m->reg_rows_cap < cap) {  // the first call, or the table has grown
        if (m->reg_rows && hipStreamSynchronize(st) != hipSuccess) return SP_ERR_HIP;  // (a kernel may still read the old rows)
        (void)hipFree(m->reg_rows);
        m->reg_rows = nullptr;
        m->reg_rows_cap = 0;
        m->reg_generation = 0;
        const hipError_t e = hipMalloc(&m->reg_rows, cap * 3 * sizeof(float4));
        if (e != hipSuccess) { sp_set_error(hipGetErrorString(e)); m->reg_rows = nullptr; return SP_ERR_HIP; }
        m->reg_rows_cap = cap;
        // once per allocation: the rows of never-used slots are not written by the kernel and not read by anyone
        if (const int rc = zero_async(m->reg_rows, cap * 3 * sizeof(float4), st); rc != SP_OK) return rc;
    }
    const unsigned blocks = div_up(cap, kBlock);
    if (reg_type == SP_REG_POINT_TO_DISTRIBUTION)
        vhm_registration_rows_kernel<true><<<blocks, kBlock, 0, st>>>(m->t, m->min_num_point, m->reg_rows);
    else
        vhm_registration_rows_kernel<false><<<blocks, kBlock, 0, st>>>(m->t, m->min_num_point, m->reg_rows);
    const int rc = launch_status();
    if (rc == SP_OK) { m->reg_generation = m->generation; m->reg_type = reg_type; }
    return rc;
}

extern "C" int sp_vhm_registration_ready(const sp_voxel_hash_map* m, int reg_type) {
    return m && sp::rows_ready(m, reg_type) ? 1 : 0;
}

extern "C" size_t sp_vhm_registration_workspace_bytes(size_t n) { return sp::vhm_workspace_bytes(n); }

extern "C" int sp_vhm_prepare_source(const float* src_covs, size_t n, int reg_type, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    using namespace sp;
    if (const int rc = check_reg_type(reg_type); rc != SP_OK) return rc;
    if (reg_type == SP_REG_POINT_TO_DISTRIBUTION || n == 0) return SP_OK;  // no source covariance in that factor
    if (!src_covs) {
        sp_set_error("[Registration::validate_params] Covariance matrices of source and target must be pre-computed before "
                     "performing GICP matching.");
        return SP_ERR_RUNTIME;
    }
    if (n >= (1ull << 32)) return invalid("[VoxelHashMap registration] more than 2^32 source points");
    if (const int rc = check_vhm_workspace(workspace, workspace_bytes, n); rc != SP_OK) return rc;
    vhm_source_rows_kernel<<<div_up(n, kBlock), kBlock, 0, as_stream(stream)>>>(reinterpret_cast<const float4*>(src_covs), (unsigned)n,
                                                                                ws_source_rows(workspace, n));
    return launch_status();
}

extern "C" int sp_vhm_neighbor_offsets_host(int neighbor_voxels, int32_t* out) {
    if (!out) return SP_ERR_INVALID_ARGUMENT;
    if (neighbor_voxels != 1 && neighbor_voxels != 7 && neighbor_voxels != 27)
        return sp::invalid("[VoxelHashMap registration] neighbor_voxels must be 1, 7 or 27");
    for (int j = 0; j < neighbor_voxels; ++j)
        for (int a = 0; a < 3; ++a) out[3 * j + a] = sp::kCellOffsets.d[j][a];
    return SP_OK;
}

extern "C" int sp_vhm_linearize(const sp_voxel_hash_map* m, const float* src_points, size_t n, const float* transT,
                                int transT_on_device, const sp_factor_params* params, int neighbor_voxels, sp_linearized* out,
                                uint64_t* corr_keys_out_opt, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace sp;
    if (const int rc = check_call("[sp_vhm_linearize] the registration rows are not those of the map as it is now and of this "
                                  "reg_type: call sp_vhm_prepare_registration", m, src_points, n, params, out); rc != SP_OK)
        return rc;
    if (neighbor_voxels != 1 && neighbor_voxels != 7 && neighbor_voxels != 27)
        return invalid("[VoxelHashMap registration] neighbor_voxels must be 1, 7 or 27");
    hipStream_t st = as_stream(stream);
    if (n == 0) return zero_async(out, sizeof(sp_linearized), st);
    if (const int rc = check_vhm_workspace(workspace, workspace_bytes, n); rc != SP_OK) return rc;
    const VhmRegArgs A = make_args(m, src_points, n, transT, transT_on_device, params, workspace, corr_keys_out_opt);
    const unsigned grid = vhm_reduce_grid(n);
    float* partials = static_cast<float*>(workspace);
    const int rc = with_loss(params->robust_type, [&](auto L) {
        return with_bool<false>(params->reg_type == SP_REG_POINT_TO_DISTRIBUTION, [&](auto P2D) {
            constexpr int loss = decltype(L)::value;
            if (neighbor_voxels == 1) vhm_linearize_kernel<loss, P2D, 1><<<grid, kBlock, 0, st>>>(A, partials);
            else if (neighbor_voxels == 7) vhm_linearize_kernel<loss, P2D, 7><<<grid, kBlock, 0, st>>>(A, partials);
            else vhm_linearize_kernel<loss, P2D, 27><<<grid, kBlock, 0, st>>>(A, partials);
            return SP_OK;
        });
    });
    if (rc != SP_OK) return rc;
    m->lin_workspace = workspace;
    m->lin_n = n;
    m->lin_generation = m->generation;
    vhm_final_reduce_kernel<<<1, kFinalThreads, 0, st>>>(partials, grid, kAcc - 1, out);
    return launch_status();
}

extern "C" int sp_vhm_error(const sp_voxel_hash_map* m, const float* src_points, size_t n, const float* transT_trial,
                            int trial_on_device, const sp_factor_params* params, sp_linearized* out, void* workspace,
                            size_t workspace_bytes, void* stream) {
    using namespace sp;
    if (const int rc = check_call("[sp_vhm_error] the registration rows are not those of the map as it is now and of this "
                                  "reg_type: call sp_vhm_prepare_registration and linearise again", m, src_points, n, params, out);
        rc != SP_OK)
        return rc;
    hipStream_t st = as_stream(stream);
    if (n == 0) return zero_async(out, sizeof(sp_linearized), st);
    if (const int rc = check_vhm_workspace(workspace, workspace_bytes, n); rc != SP_OK) return rc;
    if (m->lin_workspace != workspace || m->lin_n != n) {
        sp_set_error("[sp_vhm_error] no frozen correspondences: call sp_vhm_linearize with this map, this workspace and these "
                     "points first");
        return SP_ERR_RUNTIME;
    }
    if (m->lin_generation != m->generation) return invalid("[sp_vhm_error] the map has changed since the linearisation");
    const VhmRegArgs A = make_args(m, src_points, n, transT_trial, trial_on_device, params, workspace, nullptr);
    const unsigned grid = vhm_reduce_grid(n);
    float* partials = static_cast<float*>(workspace);
    const int rc = with_loss(params->robust_type, [&](auto L) {
        return with_bool<false>(params->reg_type == SP_REG_POINT_TO_DISTRIBUTION, [&](auto P2D) {
            vhm_error_kernel<decltype(L)::value, P2D><<<grid, kBlock, 0, st>>>(A, partials);
            return SP_OK;
        });
    });
    if (rc != SP_OK) return rc;
    vhm_final_reduce_kernel<<<1, kFinalThreads, 0, st>>>(partials, grid, 1, out);
    return launch_status();
}
