// Registration::align from MANY initial guesses in one launch (sp_gicp_align_batch): the same prepared source against the same
// prepared target from `batch` starting poses — relocalisation, start-up without a pose, a yaw sweep, loop-closure checks. The
// reference has no such call: it would run align() (registration.hpp:201-276, with pipeline/robust.hpp:78-111 around it) once
// per guess.
//
// gicp_optimize_batch_kernel is the one-workgroup-per-guess shell of sp_optimize_batch.h (the launch shape and why no workgroup
// ever waits for another are explained there) around gicp_optimize_kernel's per-lane point bodies: fused_point to linearise,
// error_prepared_point for an LM / dog-leg trial. What a hypothesis owns are the correspondence-cache rows it freezes its trials
// on, 3 x float4 per point at rows + b * 3 * n in the caller's workspace; the source tiles and the target are read-only, and the
// prepared source's own cache rows and flags are neither read nor written.
#include <cmath>

#include "sp_optimize_batch.h"

namespace sp {
namespace {

struct BatchArgs : BatchCommon {
    float4* rows;  // batch x 3 n float4: the hypotheses' correspondence-cache rows
};

template <int LOSS, bool FAST_NN, bool P2D>
struct GicpBatchProblem {
    FusedParams& P;
    float4* rows;
    __device__ __forceinline__ unsigned n() const { return P.n; }
    __device__ __forceinline__ void hypothesis(size_t b) { P.ccache = rows + b * 3 * (size_t)P.n; }
    __device__ __forceinline__ void scale(float s) { P.scale = s; }
    __device__ __forceinline__ void cache_valid(int v) { P.cache_valid = v; }
    __device__ __forceinline__ void linearize(const Rigid& T, unsigned i, float (&acc)[kAcc - 1], unsigned& cnt, unsigned& searched) {
        fused_point<LOSS, FAST_NN, P2D, kSeedSearches, kNegCert>(P, T, i, acc, cnt, searched);
    }
    __device__ __forceinline__ void error(const Rigid& T, const Rigid& TL, unsigned i, float (&acc)[1], unsigned& cnt) {
        error_prepared_point<LOSS, P2D>(P, T, TL, i, acc, cnt);
    }
    __device__ __forceinline__ unsigned searched(const float* tot) const { return (unsigned)tot[kAcc]; }  // (a float value)
};

// 256 lanes while every point has a lane (256 registers a lane), 1024 beyond (128): the two budgets of gicp_optimize_kernel, and
// its inlining rule: at 1024 lanes the state machine is a real function (CALLS).
template <int LOSS, bool FAST_NN, bool P2D, int BLOCK>
__global__ __launch_bounds__(BLOCK) void gicp_optimize_batch_kernel(FusedParams P, BatchArgs A) {
    GicpBatchProblem<LOSS, FAST_NN, P2D> Q{P, A.rows};
    optimize_batch_workgroup<BLOCK, (BLOCK > 256)>(Q, A);
}

// 3 x float4 per point and hypothesis; 0 outside the ranges the header names.
size_t batch_rows_bytes(size_t n, size_t batch) {
    if (n == 0 || n > (size_t)SP_ALIGN_BATCH_MAX_POINTS || batch == 0 || batch > (size_t)SP_ALIGN_BATCH_MAX) return 0;
    return batch * n * 3 * sizeof(float4);
}

}  // namespace
}  // namespace sp

extern "C" size_t sp_gicp_align_batch_workspace_bytes(size_t n, size_t batch) { return sp::batch_rows_bytes(n, batch); }

extern "C" int sp_gicp_align_batch(const sp_gicp_target* target, const sp_gicp_source* source, const float* T_init_device,
                                   float* T_out_device, size_t batch, const sp_factor_params* params, const sp_opt_params* opt,
                                   const float* robust_scales, int n_levels, sp_align_result* results_device, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    using namespace sp;
    if (!target || !source || !params || !opt || !T_init_device || !T_out_device || !results_device || !robust_scales)
        return invalid("[sp_gicp_align_batch] null argument");
    hipStream_t st = as_stream(stream);
    if (const int rc = check_opt_args("sp_gicp_align_batch", opt, n_levels, "the results are the initial guesses"); rc != SP_OK) return rc;
    if (const int rc = check_prepared_reg(target, params); rc != SP_OK) return rc;
    if (batch == 0 || batch > (size_t)SP_ALIGN_BATCH_MAX) return invalid("[sp_gicp_align_batch] batch must be in 1..SP_ALIGN_BATCH_MAX");
    const size_t n = source->n;
    if (n == 0 || n > (size_t)SP_ALIGN_BATCH_MAX_POINTS)
        return invalid("[sp_gicp_align_batch] the prepared source must hold 1..SP_ALIGN_BATCH_MAX_POINTS points");
    if (!workspace || workspace_bytes < batch_rows_bytes(n, batch))
        return invalid("[sp_gicp_align_batch] workspace too small (sp_gicp_align_batch_workspace_bytes)");
    if (!sp_gicp_target_has_certificates(target))  // (trial steps freeze on cache rows, and only a certified target has them)
        return invalid("[sp_gicp_align_batch] the prepared target has no reuse certificates (sp_gicp_target_certify)");
    target->note(st);
    const FusedParams P = make_fused_params(target, source, params, T_init_device, 1, nullptr, nullptr);
    BatchArgs A;
    A.rows = static_cast<float4*>(workspace);
    A.T_init = T_init_device;
    A.T_out = T_out_device;
    A.opt = *opt;
    fill_level_scales(A.scales, robust_scales, n_levels);
    A.n_levels = n_levels;
    A.reuse = source->opt_reuse ? 1 : 0;
    A.results = results_device;
    const int rc = with_variant(params->robust_type, source_fast_nn(source), params->reg_type == SP_REG_POINT_TO_DISTRIBUTION,
                                [&](auto L, auto FAST_NN, auto P2D) {
        constexpr int loss = L;
        constexpr bool fast_nn = FAST_NN, p2d = P2D;
        return with_bool<false>(n <= 256, [&](auto SMALL) {
            constexpr int B = decltype(SMALL)::value ? 256 : kAlignBlock;
            gicp_optimize_batch_kernel<loss, fast_nn, p2d, B><<<(unsigned)batch, B, 0, st>>>(P, A);
            return SP_OK;
        });
    });
    if (rc != SP_OK) return rc;
    return launch_status();
}

// Registration::best_of: the hypothesis with the most inliers among the blocks of alignments that ended properly (status 0, a
// finite pose and error, at least one inlier); ties to the smaller error, then to the lower index. Host memory only.
extern "C" int sp_align_best_host(const sp_align_result* results_host, size_t batch, size_t* best_out) {
    if (!best_out || (!results_host && batch != 0)) {
        sp_set_error("[sp_align_best_host] null argument");
        return SP_ERR_INVALID_ARGUMENT;
    }
    size_t best = batch;
    for (size_t i = 0; i < batch; ++i) {
        const sp_align_result& r = results_host[i];
        bool ok = r.status == 0u && r.inlier > 0u && std::isfinite(r.error);
        for (int k = 0; k < 16 && ok; ++k) ok = std::isfinite(r.T[k]);
        if (!ok) continue;
        if (best == batch || r.inlier > results_host[best].inlier ||
            (r.inlier == results_host[best].inlier && r.error < results_host[best].error))
            best = i;
    }
    *best_out = best;
    return SP_OK;
}
