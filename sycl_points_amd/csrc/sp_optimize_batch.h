// The device-resident optimiser's workgroup shell: what gicp_optimize_kernel (registration_opt.hip), gicp_optimize_batch_kernel
// (registration_batch.hip) and vhm_optimize_batch_kernel (voxel_registration_batch.hip) do around their point loops. All three
// fill the OptState in LDS the same way (opt_state_init) and leave the same result block (opt_publish_block), whose done flag is
// the one thing a caller may wait on (opt_publish_done): the C++ facade and the Python package spin on it in host-mapped memory.
//
// optimize_batch_workgroup is the whole program of the two batch kernels, one workgroup per initial guess. The launch is a plain
// grid of `batch` workgroups; workgroup b runs the WHOLE alignment of hypothesis b the way a one-workgroup launch of
// gicp_optimize_kernel does: a step is a pass of the workgroup's lanes over the source (Problem::linearize, or Problem::error for
// an LM / dog-leg trial over the correspondences the linearisation froze), the step's totals are summed in LDS
// (block_reduce_lds), and one lane runs the optimiser's state machine (sp_optimizer.h) on LDS. Hypotheses share nothing they
// write: every input is read-only, and what a hypothesis freezes its trials on (cache rows, slots) is its own part of the caller's
// workspace, which Problem::hypothesis(b) selects. So no workgroup ever waits for another one: no counter, no residency
// requirement, no bounded wait, any batch size on any stream (a capturing one included). Every loop is bounded: max_iterations,
// lm_max_inner_iterations, SP_OPT_MAX_LEVELS, and whatever bounds the Problem's own per-point bodies.
//
// A Problem supplies, all inlined:
//   n()                                  source points
//   hypothesis(b)                        point the per-point arguments at hypothesis b's own rows
//   scale(s)                             the robust scale of the level
//   cache_valid(v)                       whether this linearisation may trust the hypothesis's rows
//   linearize(T, i, acc, cnt, searched)  point i at pose T into the 28 sums and the inlier count
//   error(T, TL, i, acc, cnt)            point i's robust error at the trial pose T over the correspondence frozen at TL
//   searched(tot)                        how many points the linearisation whose totals these are looked up
#ifndef SP_OPTIMIZE_BATCH_H
#define SP_OPTIMIZE_BATCH_H

#include "sp_optimizer.h"

namespace sp {
namespace {

// OptState in LDS before the first step. The caller places the __syncthreads() behind it.
__device__ __forceinline__ void opt_state_init(OptState& S, const float* T_init, const sp_opt_params& opt, int n_levels, int reuse,
                                               int cache_valid, sp_align_result* result) {
    if (threadIdx.x < 16) {
        const float v = T_init[threadIdx.x];
        S.sT[threadIdx.x] = v;
        S.sTlin[threadIdx.x] = v;
    } else if (threadIdx.x == 32) {
        OptCtl c;
        opt_start(c, opt, cache_valid);
        S.ctl = c;
        S.opt = opt;
        S.n_levels = n_levels;
        S.reuse = reuse;
        S.result = result;
    } else if (threadIdx.x >= 64 && threadIdx.x < 64 + 48) {
        reinterpret_cast<float*>(&S.slin)[threadIdx.x - 64] = 0.0f;
    }
}

// The result block: RegistrationResult of the last level + the linearisation pose + counters (pad[0], the done flag, is
// opt_publish_done's).
__device__ __forceinline__ void opt_publish_block(const OptState& S, sp_align_result* r, float* T_out) {
    const unsigned t = threadIdx.x;
    if (t < 16) { r->T[t] = S.sT[t]; T_out[t] = S.sT[t]; }
    else if (t < 32) r->T_lin[t - 16] = S.sTlin[t - 16];
    else if (t >= 64 && t < 100) r->H[t - 64] = S.slin.H[t - 64];
    else if (t >= 128 && t < 134) r->b[t - 128] = S.slin.b[t - 128];
    else if (t == 192) opt_result_scalars(S, r);
}

// The block is complete: the flag goes last, behind a system-scope release — the block may be host-mapped memory whose pad[0]
// the caller cleared and spins on (no read-back copy, no synchronisation).
__device__ __forceinline__ void opt_publish_done(sp_align_result* r) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system();
        __hip_atomic_store(&r->pad[0], (unsigned)SP_ALIGN_RESULT_DONE, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// What every batch launch is given beside its Problem's own arguments.
struct BatchCommon {
    const float* T_init;   // device: batch x 16, column-major
    float* T_out;          // device: batch x 16 (may alias T_init: workgroup b reads its pose before it writes anything)
    sp_opt_params opt;
    float scales[SP_OPT_MAX_LEVELS];
    int n_levels;
    int reuse;             // later linearisations may trust the hypothesis's rows
    sp_align_result* results;
};

// The step's totals (block_reduce_lds: sums | uint32 count | ...) into the state machine.
__device__ __forceinline__ void batch_after_linearize(OptState& S, const float* tot, unsigned searched) {
    unpack_totals(tot, kAcc - 1, &S.slin);
    ++S.ctl.n_lin;
    S.ctl.searched += searched;
    opt_after_linearize(S, true);
}
__device__ __forceinline__ void batch_after_trial(OptState& S, const float* tot) {
    opt_after_trial(S, tot[0], __float_as_uint(tot[1]), true);
}
// (CALLS: real functions, as in the 1024-lane instantiations of gicp_optimize_kernel: inlined, the state machine takes the point
// loops' registers with it)
__device__ __noinline__ void batch_after_linearize_call(OptState& S, const float* tot, unsigned searched) {
    batch_after_linearize(S, tot, searched);
}
__device__ __noinline__ void batch_after_trial_call(OptState& S, const float* tot) { batch_after_trial(S, tot); }

template <int BLOCK, bool CALLS, class Problem>
__device__ __forceinline__ void optimize_batch_workgroup(Problem& Q, const BatchCommon& A) {
    __shared__ OptState S;
    __shared__ float tot[kPartial];
    const size_t b = blockIdx.x;
    sp_align_result* const result = A.results + b;
    Q.hypothesis(b);
    opt_state_init(S, A.T_init + b * 16, A.opt, A.n_levels, A.reuse, 0, result);  // the rows hold nothing yet
    __syncthreads();
    for (;;) {
        const int phase = S.ctl.phase;  // uniform over the workgroup
        Q.scale(A.scales[S.ctl.level]);
        if (phase == PHASE_LIN) {
            Q.cache_valid(S.ctl.cache_valid);
            const Rigid T = uniform_pose(S.sT);
            float acc[kAcc - 1];
            unsigned cnt = 0, searched = 0;
#pragma unroll
            for (int e = 0; e < kAcc - 1; ++e) acc[e] = 0.0f;
            for (unsigned i = threadIdx.x; i < Q.n(); i += BLOCK) Q.linearize(T, i, acc, cnt, searched);
            block_reduce_lds<kAcc - 1, BLOCK>(acc, cnt, searched, tot);
        } else {  // PHASE_TRIAL: the lane that linearised a point also evaluates it
            const Rigid T = uniform_pose(S.sTt);
            const Rigid TL = uniform_pose(S.sTlin);
            float acc[1] = {0.0f};
            unsigned cnt = 0;
            for (unsigned i = threadIdx.x; i < Q.n(); i += BLOCK) Q.error(T, TL, i, acc, cnt);
            block_reduce_lds<1, BLOCK>(acc, cnt, 0u, tot);
        }
        if (threadIdx.x == 0) {
            if constexpr (!CALLS) {
                if (phase == PHASE_LIN) batch_after_linearize(S, tot, Q.searched(tot));
                else batch_after_trial(S, tot);
            } else {
                if (phase == PHASE_LIN) batch_after_linearize_call(S, tot, Q.searched(tot));
                else batch_after_trial_call(S, tot);
            }
        }
        __syncthreads();
        if (S.ctl.done) break;
    }
    opt_publish_block(S, result, A.T_out + b * 16);
    opt_publish_done(result);
}

}  // namespace
}  // namespace sp
#endif
