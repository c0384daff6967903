// Registration::align from MANY initial guesses in one launch (sp_gicp_align_batch): the same prepared source against the same
// prepared target from `batch` starting poses — relocalisation, start-up without a pose, a yaw sweep, loop-closure checks. The
// reference has no such call: it would run align() (registration.hpp:201-276, with pipeline/robust.hpp:78-111 around it) once
// per guess.
//
// gicp_optimize_batch_kernel is a plain grid of `batch` workgroups; workgroup b runs the WHOLE alignment of hypothesis b the way
// a one-workgroup launch of gicp_optimize_kernel does (registration_opt.hip): a step is a pass of the workgroup's lanes over the
// source (fused_point to linearise, error_prepared_point for an LM / dog-leg trial), the step's totals are summed in LDS
// (block_reduce_lds), and one lane runs the optimiser's state machine (sp_optimizer.h) on LDS. Hypotheses share nothing they
// write: the source tiles and the target are read-only, and the correspondence-cache rows a hypothesis freezes its trials on
// are its own, 3 x float4 per point at rows + b * 3 * n in the caller's workspace. So no workgroup ever waits for another one:
// no counter, no residency requirement, no bounded wait, any batch size on any stream (a capturing one included), and the
// prepared source's own cache rows and flags are neither read nor written.
#include <cmath>

#include "sp_optimizer.h"

namespace sp {
namespace {

struct BatchArgs {
    float4* rows;          // batch x 3 n float4: the hypotheses' correspondence-cache rows
    const float* T_init;   // device: batch x 16, column-major
    float* T_out;          // device: batch x 16 (may alias T_init: workgroup b reads its pose before it writes anything)
    sp_opt_params opt;
    float scales[SP_OPT_MAX_LEVELS];
    int n_levels;
    int reuse;             // later linearisations may trust the hypothesis's rows under the target's certificates
    sp_align_result* results;
};

// The step's totals (block_reduce_lds: sums | uint32 count | searched as a float value) into the state machine.
__device__ __forceinline__ void batch_after_linearize(OptState& S, const float* tot) {
    unpack_totals(tot, kAcc - 1, &S.slin);
    ++S.ctl.n_lin;
    S.ctl.searched += (unsigned)tot[kAcc];
    opt_after_linearize(S, true);
}
__device__ __forceinline__ void batch_after_trial(OptState& S, const float* tot) {
    opt_after_trial(S, tot[0], __float_as_uint(tot[1]), true);
}
// (real functions in the 1024-lane instantiations, as in gicp_optimize_kernel: inlined, the state machine takes the point loops'
// registers with it)
__device__ __noinline__ void batch_after_linearize_call(OptState& S, const float* tot) { batch_after_linearize(S, tot); }
__device__ __noinline__ void batch_after_trial_call(OptState& S, const float* tot) { batch_after_trial(S, tot); }

template <int LOSS, bool FAST_NN, bool P2D, int BLOCK>
__global__ __launch_bounds__(BLOCK) void gicp_optimize_batch_kernel(FusedParams P, BatchArgs A) {
    __shared__ OptState S;
    __shared__ float tot[kPartial];
    const size_t b = blockIdx.x;
    sp_align_result* const result = A.results + b;
    P.ccache = A.rows + b * 3 * (size_t)P.n;
    if (threadIdx.x < 16) {
        const float v = A.T_init[b * 16 + threadIdx.x];
        S.sT[threadIdx.x] = v;
        S.sTlin[threadIdx.x] = v;
    } else if (threadIdx.x == 32) {
        OptCtl c;
        opt_start(c, A.opt, 0);  // the rows hold nothing yet: the first linearisation searches every point
        S.ctl = c;
        S.opt = A.opt;
        S.n_levels = A.n_levels;
        S.reuse = A.reuse;
        S.result = result;
    } else if (threadIdx.x >= 64 && threadIdx.x < 64 + 48) {
        reinterpret_cast<float*>(&S.slin)[threadIdx.x - 64] = 0.0f;
    }
    __syncthreads();
    for (;;) {
        const int phase = S.ctl.phase;  // uniform over the workgroup
        P.scale = A.scales[S.ctl.level];
        if (phase == PHASE_LIN) {
            P.cache_valid = S.ctl.cache_valid;
            const Rigid T = uniform_pose(S.sT);
            float acc[kAcc - 1];
            unsigned cnt = 0, searched = 0;
#pragma unroll
            for (int e = 0; e < kAcc - 1; ++e) acc[e] = 0.0f;
            for (unsigned i = threadIdx.x; i < P.n; i += BLOCK)
                fused_point<LOSS, FAST_NN, P2D, kSeedSearches, kNegCert>(P, T, i, acc, cnt, searched);
            block_reduce_lds<kAcc - 1, BLOCK>(acc, cnt, searched, tot);
        } else {  // PHASE_TRIAL: the lane that searched for a point also evaluates it
            const Rigid T = uniform_pose(S.sTt);
            const Rigid TL = uniform_pose(S.sTlin);
            float acc[1] = {0.0f};
            unsigned cnt = 0;
            for (unsigned i = threadIdx.x; i < P.n; i += BLOCK) error_prepared_point<LOSS, P2D>(P, T, TL, i, acc, cnt);
            block_reduce_lds<1, BLOCK>(acc, cnt, 0u, tot);
        }
        if (threadIdx.x == 0) {
            if constexpr (BLOCK <= 256) {
                if (phase == PHASE_LIN) batch_after_linearize(S, tot);
                else batch_after_trial(S, tot);
            } else {
                if (phase == PHASE_LIN) batch_after_linearize_call(S, tot);
                else batch_after_trial_call(S, tot);
            }
        }
        __syncthreads();
        if (S.ctl.done) break;
    }
    // RegistrationResult of the last level + the linearisation pose + counters; the done flag goes last, behind a system-scope
    // release, as the single launch stores it (the blocks may be host-mapped memory)
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
    if (!target || !source || !params || !opt || !T_init_device || !T_out_device || !results_device || !robust_scales) {
        sp_set_error("[sp_gicp_align_batch] null argument");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    if (n_levels < 1 || n_levels > SP_OPT_MAX_LEVELS) {
        sp_set_error("[sp_gicp_align_batch] n_levels must be in 1..SP_OPT_MAX_LEVELS");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (opt->method != SP_OPT_GAUSS_NEWTON && opt->method != SP_OPT_LEVENBERG_MARQUARDT && opt->method != SP_OPT_POWELL_DOGLEG) {
        sp_set_error("[sp_gicp_align_batch] unknown optimization method");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (opt->max_iterations < 1 || opt->max_iterations > 65535) {
        sp_set_error("[sp_gicp_align_batch] max_iterations must be in 1..65535 (0 iterations: the results are the initial guesses)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (const int rc = check_prepared_reg(target, params); rc != SP_OK) return rc;
    if (batch == 0 || batch > (size_t)SP_ALIGN_BATCH_MAX) {
        sp_set_error("[sp_gicp_align_batch] batch must be in 1..SP_ALIGN_BATCH_MAX");
        return SP_ERR_INVALID_ARGUMENT;
    }
    const size_t n = source->n;
    if (n == 0 || n > (size_t)SP_ALIGN_BATCH_MAX_POINTS) {
        sp_set_error("[sp_gicp_align_batch] the prepared source must hold 1..SP_ALIGN_BATCH_MAX_POINTS points");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (!workspace || workspace_bytes < batch_rows_bytes(n, batch)) {
        sp_set_error("[sp_gicp_align_batch] workspace too small (sp_gicp_align_batch_workspace_bytes)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (!sp_gicp_target_has_certificates(target)) {  // (trial steps freeze on cache rows, and only a certified target has them)
        sp_set_error("[sp_gicp_align_batch] the prepared target has no reuse certificates (sp_gicp_target_certify)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    target->note(st);
    const FusedParams P = make_fused_params(target, source, params, T_init_device, 1, nullptr, nullptr);
    BatchArgs A;
    A.rows = static_cast<float4*>(workspace);
    A.T_init = T_init_device;
    A.T_out = T_out_device;
    A.opt = *opt;
    for (int l = 0; l < SP_OPT_MAX_LEVELS; ++l) A.scales[l] = robust_scales[l < n_levels ? l : n_levels - 1];
    A.n_levels = n_levels;
    A.reuse = source->opt_reuse ? 1 : 0;
    A.results = results_device;
    // 256 lanes while every point has a lane (256 registers a lane), 1024 beyond (128): the two budgets of gicp_optimize_kernel
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
