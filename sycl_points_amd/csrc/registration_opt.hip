// Registration::align's optimiser loop on the device, for every OptimizationMethod, with the robust-scale annealing of
// pipeline::RobustAligner around it (replaces registration.hpp:201-276, 803-828, 830-895, 897-964, dogleg_step.hpp:35-101 and
// pipeline/robust.hpp:78-111 for the prepared GICP / point-to-distribution path): ONE launch, ONE read-back per alignment.
//
// The reference drives LM and dog-leg from the host: per outer iteration one search + K11 (submit, wait, toCPU) and per trial
// step a solve on the host, a K12 launch with two freshly allocated USM vectors, another wait (registration.hpp:674-675,
// 685-686, 854). Its own example — LM, Geman-McClure, three annealing levels on a 1000-point random sample
// (example_registration.cpp:29-55) — is about sixty such round trips for work that one compute unit finishes in microseconds.
//
// gicp_optimize_kernel is a persistent launch of up to 256 workgroups (256 lanes each up to 64 K source points, 1024 beyond:
// see the note above the kernel). A STEP is a pass over the source:
//   linearise  fused_point of the per-iteration Gauss-Newton kernel (certificate -> cached correspondence, else exact NN on
//              the grid; 28 sums + inlier count)                                                -> one partial row per workgroup
//   trial      error_prepared_point: K12 at the trial pose over the cache rows (frozen correspondences) -> one partial row
// Between steps every workgroup waits for all rows (grid_arrive / grid_wait, registration_device.h: the hand-off
// gicp_align_persistent_kernel uses), sums them in reduce_rows_1024's fixed order and lets ONE lane run the optimiser's state
// machine (opt_after_*) on LDS: every workgroup takes the same decisions from the same bits, so nothing is broadcast. A launch of ONE workgroup (up to 1024 points: the reference pipeline's default
// random sample) keeps its totals in LDS and touches no counter.
// Rows ping-pong by step parity: a workgroup can only write the row of step s + 1 after every workgroup has stored the row
// of step s, i.e. after every workgroup has finished reading the rows of step s - 1 that it overwrites.
#include <algorithm>

#include "sp_optimize_batch.h"

namespace sp {
namespace {

struct OptArgs {
    float* part[2];
    unsigned* tickets;
    unsigned long long* trows[2];  // WAVEQ: tagged partial rows, by step parity
    unsigned tag_base;             // WAVEQ: this launch's epoch << 20 (tags of earlier launches never match: no zeroing per launch)
    float4* rows[2];               // cache rows: [0] the source's own (what the launch leaves), [1] the other set of fused steps
    float4* qcert[2];              // WAVEQ: the margin certificates beside them (null: none)
    int qcert_trusted;             // ... and whether those of set 0 belong to its rows as the launch finds them
    int fuse;                      // trial steps also linearise (PHASE_FUSED)
    const float* T_init;          // device: initial guess
    float* T_out;                 // device: final pose (may alias T_init: it is read before anything is written)
    sp_opt_params opt;
    float scales[SP_OPT_MAX_LEVELS];
    int n_levels;
    int reuse;                    // later linearisations may trust the correspondence cache
    sp_align_result* result;
    unsigned long long budget;    // wall_clock64 ticks a wait may take
};

// After a linearisation step: tot = 28 sums, the uint32 count, the searched count as a float value.
__device__ __forceinline__ void opt_after_linearize_impl(OptState& S, const float* tot, bool publish) {
    unpack_totals(tot, kAcc - 1, &S.slin);
    ++S.ctl.n_lin;
    S.ctl.searched += (unsigned)tot[kAcc];
    opt_after_linearize(S, publish);
}

// After a trial step: tot[0] = the robust error at the trial pose, tot[1] = the uint32 inlier count.
__device__ __forceinline__ void opt_after_trial_impl(OptState& S, const float* tot, bool publish) {
    opt_after_trial(S, tot[0], __float_as_uint(tot[1]), publish);
}

// The state machine as real functions (the 1024-lane instantiations: inlined it takes the point loops' registers with it, 90
// spilled VGPRs) and inlined (the 256-lane instantiations have 256 registers: 5.5 -> 1.5 us per linearisation step).
// After a fused step: tot[0..29] the linearisation at the trial pose (sums | count | searched), tot[30] / tot[31] the trial's
// robust error / inlier count. The trial is decided exactly as a plain trial step decides it; when its pose was taken and what
// follows is the linearisation that was speculated on (same pose, the level whose scale it used), that linearisation is adopted
// as if its step had just run: the same sequence of state-machine calls as the unfused loop, one hand-off less.
__device__ __forceinline__ void opt_after_fused_impl(OptState& S, const float* tot, bool publish) {
    OptCtl& c = S.ctl;
    const float trial[2] = {tot[30], tot[31]};
    opt_after_trial_impl(S, trial, publish);
    if (!c.done && c.took && c.phase == PHASE_LIN && c.level == c.spec_level) {
        c.cur ^= 1;  // the rows the speculative linearisation wrote are the correspondences now
        opt_after_linearize_impl(S, tot, publish);
    }
}
// A trial is due: make it a fused step when there is a linearisation to speculate on (an accepted trial that ends the last level
// is followed by nothing).
__device__ __forceinline__ void opt_upgrade_trial(OptState& S, int fuse) {
    OptCtl& c = S.ctl;
    if (!fuse || c.done || c.phase != PHASE_TRIAL) return;
    const int next = (c.conv_any || c.iter + 1 >= S.opt.max_iterations) ? c.level + 1 : c.level;
    if (next < S.n_levels) { c.phase = PHASE_FUSED; c.spec_level = next; }
}
__device__ __noinline__ void opt_after_linearize_call(OptState& S, const float* tot, bool publish) { opt_after_linearize_impl(S, tot, publish); }
__device__ __noinline__ void opt_after_trial_call(OptState& S, const float* tot, bool publish) { opt_after_trial_impl(S, tot, publish); }

// BLOCK: lanes per workgroup. The search of a linearisation is bound by vector issue (thousands of wave instructions per 64
// points), so a SMALL source wants its waves on many compute units, each wave alone on its SIMD — workgroups of 256 lanes —
// and pays for it with the arrival counter between steps; a large source fills every compute unit with 1024 lanes anyway.
// The hand-off between two steps of a wave-per-point launch (up to 256 small workgroups, a step of a few microseconds: the
// counter hand-off — drain the row's stores, count in, poll the counter, read all rows: three dependent trips to memory —
// costs more than the step). Here a row is 32 granules {value, tag = step + 1} and each granule travels in ONE 8-byte store
// (the exchange slots' trick, comm.hip): a reader polls the rows themselves, every lane its share of granules, all loads of a
// round in flight together; a round in which every tag matches IS the data. Rows ping-pong by step parity as the counter form's
// do. A tag is (epoch of the launch) << 20 | (step + 1) mod 2^20: the buffer is zeroed when the source is created and when the
// 12-bit epoch wraps, never per launch (a row is rewritten by its owner every second step, so a stale tag is at most two steps old).
// Sums in a fixed order (lane (group, slot): rows group, group + G, ... in order; then the groups in order): the same bits in
// every workgroup. On return red[0][e] holds the totals (slot nv the uint32 count); false: the wait ran out.
template <int BLOCK>
__device__ __forceinline__ bool tagged_rows_exchange(unsigned long long* rows, unsigned tag, float mine, unsigned grid, int nv,
                                                     float (*red)[kPartial], unsigned long long budget, unsigned* s_wait,
                                                     unsigned more_counts = 0u) {
    constexpr unsigned kGroups = BLOCK / 32;
    constexpr int kPer = kAlignMaxBlocks / (int)kGroups;
    const unsigned e = threadIdx.x & 31u, grp = threadIdx.x >> 5;
    if (threadIdx.x < 32)
        __hip_atomic_store(rows + (size_t)blockIdx.x * 32 + e, ((unsigned long long)tag << 32) | __float_as_uint(mine),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool is_count = (int)e == nv || ((more_counts >> e) & 1u) != 0u;  // (slots summed as uint32 counts)
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        unsigned long long g[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const unsigned r = grp + (unsigned)j * kGroups;
            g[j] = r < grid ? __hip_atomic_load(rows + (size_t)r * 32 + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                            : ((unsigned long long)tag << 32);
        }
        bool ok = true;
        float sum = 0.0f;
        unsigned c = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            ok = ok && (unsigned)(g[j] >> 32) == tag;
            const unsigned bits = (unsigned)g[j];
            if (is_count) c += bits;
            else sum += __uint_as_float(bits);
        }
        if (__syncthreads_and(ok ? 1 : 0)) {
            red[grp][e] = is_count ? __uint_as_float(c) : sum;
            break;
        }
        if (threadIdx.x == 0) *s_wait = (wall_clock64() - t0 > budget) ? 2u : 0u;
        __syncthreads();
        if (*s_wait == 2u) return false;
        __builtin_amdgcn_s_sleep(1);
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        float t = 0.0f;
        unsigned ct = 0;
#pragma unroll
        for (unsigned p = 0; p < kGroups; ++p) {
            const float v = red[p][e];
            if (is_count) ct += __float_as_uint(v);
            else t += v;
        }
        red[0][e] = is_count ? __uint_as_float(ct) : t;
    }
    __syncthreads();
    return true;
}
// A workgroup's totals of a wave-per-point step: every lane of a wave holds the wave's sums, so lane 0 of each wave hands them
// over and lane e < 32 returns slot e of the workgroup's row (sums | uint32 count bits | searched as a float value | zeros).
// A fused step (NV = 28) also hands over its trial: slot 30 the robust error (a float sum), slot 31 the inlier count (uint32 bits).
template <int NV, int BLOCK>
__device__ __forceinline__ float waveq_row_slot(const float (&acc)[NV], unsigned cnt, unsigned extra, float (*red)[kPartial],
                                                float trial_error = 0.0f, unsigned trial_cnt = 0u) {
    const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < NV; ++e) red[wave][e] = acc[e];
        red[wave][NV] = __uint_as_float(cnt);
        red[wave][NV + 1] = __uint_as_float(extra);
        if (NV + 3 < kPartial) {
            red[wave][kPartial - 2] = trial_error;
            red[wave][kPartial - 1] = __uint_as_float(trial_cnt);
        }
    }
    __syncthreads();
    float v = 0.0f;
    if ((int)threadIdx.x < NV || (NV + 3 < kPartial && (int)threadIdx.x == kPartial - 2)) {
#pragma unroll
        for (int w = 0; w < BLOCK / kWave; ++w) v += red[w][threadIdx.x];
    } else if ((int)threadIdx.x == NV || (int)threadIdx.x == NV + 1 || (NV + 3 < kPartial && (int)threadIdx.x == kPartial - 1)) {
        unsigned c = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / kWave; ++w) c += __float_as_uint(red[w][threadIdx.x]);
        v = (int)threadIdx.x == NV + 1 ? (float)c : __uint_as_float(c);
    }
    return v;
}

// WAVEQ: one wave per source point in the linearisation steps (fused_query_wave) — sources of up to kWaveQueryMax points, spread
// over up to 256 workgroups of four waves: the step then costs a handful of dependent round trips instead of the longest
// per-lane walk through a 2x2x2 block of a surface cloud (the reference's example, 1000 points against 6 k: 16-26 us per
// linearisation per lane, a few us per wave).
// By itself (sp_gicp_source_set_wave_per_point = 1, the default) the launch takes this form up to kWaveQueryMax points, where
// every point has a wave to itself. Told to (= 2: the caller knows the target's cells are crowded — sp_grid_max_cell_points — a
// raw LiDAR scan with thousands of returns in one cell) up to kWaveQueryForcedMax: a wave then walks through n / 4096 points one
// after the other, which loses to a lane per point on a cloud of even density (20 k points in a filled box: 67 against 21 us
// per iteration) and wins where a lane's walk through its 2x2x2 block is thousands of candidates long (the reference's bundled
// scans at full resolution, 5032 returns in the sensor's own cell: 212 against 686 us; scratch/waveq_crossover.py).
constexpr size_t kWaveQueryMax = 2048, kWaveQueryForcedMax = 131072;
template <int LOSS, bool FAST_NN, bool P2D, int BLOCK, bool WAVEQ = false>
__global__ __launch_bounds__(BLOCK) void gicp_optimize_kernel(FusedParams P, OptArgs A) {
    __shared__ OptState S;
    __shared__ float red[BLOCK / 32][kPartial];
    __shared__ unsigned s_wait;
    const unsigned stride = gridDim.x * BLOCK;
    const unsigned tile = xcd_tile();
    const bool single = gridDim.x == 1;
    const bool publish = blockIdx.x == 0;
    opt_state_init(S, A.T_init, A.opt, A.n_levels, A.reuse, P.cache_valid, A.result);  // (identical in every workgroup)
    __syncthreads();
#ifdef SP_OPT_TIMING
    unsigned long long wg_t0 = 0;
#define SP_WG_BEGIN() if (threadIdx.x == 0) wg_t0 = wall_clock64()
#define SP_WG_END() if (threadIdx.x == 0 && step < 24 && blockIdx.x < 8) g_sp_wg[step * 8 + blockIdx.x] = wall_clock64() - wg_t0
#else
#define SP_WG_BEGIN()
#define SP_WG_END()
#endif
#ifdef SP_OPT_TIMING  // development builds: wall_clock64 stamps of the first steps into the tail of the result's log
    unsigned long long* const stamps = reinterpret_cast<unsigned long long*>(&A.result->log[8]);
#define SP_STAMP(k) if (publish && threadIdx.x == 0 && step < 20) stamps[step * 5 + (k)] = wall_clock64()
#else
#define SP_STAMP(k)
#endif
    for (unsigned step = 0;; ++step) {
        const int phase = S.ctl.phase;  // uniform over the grid
#ifdef SP_OPT_TIMING
        if (publish && threadIdx.x == 0) g_sp_step = step;
        __syncthreads();
#endif
        SP_STAMP(0);
        SP_WG_BEGIN();
        float* const row = A.part[step & 1] + (size_t)blockIdx.x * kPartial;
        [[maybe_unused]] float mine = 0.0f;  // WAVEQ: slot threadIdx.x < 32 of this workgroup's row
        if constexpr (WAVEQ) P.ccache = A.rows[S.ctl.cur];  // (uniform; the other kinds of launch never leave set 0)
        if (phase == PHASE_LIN) {
            P.scale = A.scales[S.ctl.level];
            P.cache_valid = S.ctl.cache_valid;
            const Rigid T = uniform_pose(S.sT);
            float acc[kAcc - 1];
            unsigned cnt = 0, searched = 0;
#pragma unroll
            for (int e = 0; e < kAcc - 1; ++e) acc[e] = 0.0f;
            if constexpr (WAVEQ) {
                const unsigned nw = BLOCK / kWave;
                const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
                // (rows that another kind of launch refreshed carry no margin certificates of their own: the launch's first
                // linearisation only writes them)
                const bool qc_trust = A.qcert_trusted || S.ctl.n_lin > 0;
                for (unsigned i = blockIdx.x * nw + wave; i < P.n; i += gridDim.x * nw)
                    fused_query_wave<LOSS, P2D>(P, T, i, acc, cnt, searched, nullptr, qc_trust ? A.qcert[S.ctl.cur] : nullptr, A.qcert[S.ctl.cur]);
                SP_STAMP(4);
                mine = waveq_row_slot<kAcc - 1, BLOCK>(acc, cnt, searched, red);
            } else if constexpr (FAST_NN && BLOCK <= 256) {  // (the staged search: open queries are finished by the whole wave)
                for (unsigned b = tile * BLOCK; b < P.n; b += stride)
                    fused_point_wave<LOSS, P2D>(P, T, b + threadIdx.x, b + threadIdx.x < P.n, acc, cnt, searched);
            } else {  // (1024 lanes: 128 registers — the per-lane stages of the per-iteration kernel fit them, the wave's tail does not)
                for (unsigned i = tile * BLOCK + threadIdx.x; i < P.n; i += stride)
                    fused_point<LOSS, FAST_NN, P2D, kSeedSearches, kNegCert>(P, T, i, acc, cnt, searched);
            }
            if constexpr (!WAVEQ) {
                SP_STAMP(4);
                if (single) block_reduce_lds<kAcc - 1, BLOCK>(acc, cnt, searched, red[0]);
                else block_reduce_store<kAcc - 1, BLOCK, true>(acc, cnt, row, false, searched);
            }
        } else if (WAVEQ && phase == PHASE_FUSED) {
            if constexpr (WAVEQ) {
                // the trial (frozen correspondences of the current rows, this level's scale) and the linearisation at its pose
                // (fresh correspondences into the OTHER rows, the scale of the level that would follow) in one pass
                const Rigid T = uniform_pose(S.sTt);
                const Rigid TL = uniform_pose(S.sTlin);
                float acc[kAcc - 1], acc_t[1] = {0.0f};
                unsigned cnt = 0, searched = 0, cnt_t = 0;
#pragma unroll
                for (int e = 0; e < kAcc - 1; ++e) acc[e] = 0.0f;
                float4* const rows_out = A.rows[S.ctl.cur ^ 1];
                const float scale_trial = A.scales[S.ctl.level], scale_lin = A.scales[S.ctl.spec_level];
                const int reuse = S.reuse;
                const unsigned nw = BLOCK / kWave;
                const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
                for (unsigned i = blockIdx.x * nw + wave; i < P.n; i += gridDim.x * nw) {
                    P.scale = scale_trial;
                    error_prepared_point<LOSS, P2D>(P, T, TL, i, acc_t, cnt_t);
                    P.scale = scale_lin;
                    P.cache_valid = reuse;
                    fused_query_wave<LOSS, P2D>(P, T, i, acc, cnt, searched, rows_out, A.qcert[S.ctl.cur], A.qcert[S.ctl.cur ^ 1]);
                }
                SP_STAMP(4);
                mine = waveq_row_slot<kAcc - 1, BLOCK>(acc, cnt, searched, red, acc_t[0], cnt_t);
            }
        } else {
            const Rigid T = uniform_pose(S.sTt);
            const Rigid TL = uniform_pose(S.sTlin);
            P.scale = A.scales[S.ctl.level];
            float acc[1] = {0.0f};
            unsigned cnt = 0;
            if constexpr (WAVEQ) {
                // the wave that searched for a point also evaluates it: a cache row is only ever touched by one wave of the launch
                // (rows written on one XCD are not visible through another XCD's L2 before the launch ends)
                const unsigned nw = BLOCK / kWave;
                const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
                for (unsigned i = blockIdx.x * nw + wave; i < P.n; i += gridDim.x * nw)
                    error_prepared_point<LOSS, P2D>(P, T, TL, i, acc, cnt);
                mine = waveq_row_slot<1, BLOCK>(acc, cnt, 0u, red);
            } else {
                for (unsigned i = tile * BLOCK + threadIdx.x; i < P.n; i += stride)
                    error_prepared_point<LOSS, P2D>(P, T, TL, i, acc, cnt);
                if (single) block_reduce_lds<1, BLOCK>(acc, cnt, 0u, red[0]);
                else block_reduce_store<1, BLOCK, true>(acc, cnt, row, false, 0u);
            }
        }
        SP_STAMP(1);
        SP_WG_END();
        auto wait_ran_out = [&] {  // (uniform per workgroup; every workgroup runs into the same bound) — loud: NaN pose, status 2
            if (publish) {
                if (threadIdx.x < 16) { A.T_out[threadIdx.x] = __int_as_float(0x7fc00000); A.result->T[threadIdx.x] = __int_as_float(0x7fc00000); }
                if (threadIdx.x == 16) { A.result->status = 2u; A.result->converged = 0u; A.result->log_entries = 0u; }
                opt_publish_done(A.result);
            }
        };
        if constexpr (WAVEQ) {
            if (single) {
                __syncthreads();
                if (threadIdx.x < 32) red[0][threadIdx.x] = mine;
                __syncthreads();
            } else if (!tagged_rows_exchange<BLOCK>(A.trows[step & 1], A.tag_base | ((step + 1u) & 0xfffffu), mine, gridDim.x,
                                                    phase == PHASE_TRIAL ? 1 : kAcc - 1, red, A.budget, &s_wait,
                                                    phase == PHASE_FUSED ? 1u << (kPartial - 1) : 0u)) {
                wait_ran_out();
                return;
            }
        } else if (!single) {
            grid_arrive(A.tickets);
            if (threadIdx.x == 0) s_wait = grid_wait(A.tickets, gridDim.x * (step + 1u), A.budget) ? 0u : 2u;
            __syncthreads();
            if (s_wait == 2) {
                wait_ran_out();
                return;
            }
            reduce_rows_block<BLOCK, true>(A.part[step & 1], gridDim.x, phase == PHASE_LIN ? kAcc - 1 : 1, red);
        }
        SP_STAMP(2);
        if (threadIdx.x == 0) {
            if constexpr (BLOCK <= 256) {
                if (phase == PHASE_LIN) opt_after_linearize_impl(S, red[0], publish);
                else if (WAVEQ && phase == PHASE_FUSED) opt_after_fused_impl(S, red[0], publish);
                else opt_after_trial_impl(S, red[0], publish);
                if constexpr (WAVEQ) opt_upgrade_trial(S, A.fuse);
            } else {
                if (phase == PHASE_LIN) opt_after_linearize_call(S, red[0], publish);
                else opt_after_trial_call(S, red[0], publish);
            }
        }
        __syncthreads();
        SP_STAMP(3);
        if (S.ctl.done) {
#ifdef SP_OPT_TIMING
            if (publish) g_sp_step = 0;
#endif
            if (publish) {  // (workgroup 0)
                opt_publish_block(S, A.result, A.T_out);
                opt_publish_done(A.result);
            }
            if constexpr (WAVEQ) {
                if (S.ctl.cur != 0) {  // the launch leaves its correspondences in the source's own rows: every wave copies its points'
                    const unsigned nw = BLOCK / kWave;
                    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
                    const unsigned lane = threadIdx.x & (kWave - 1);
                    for (unsigned i = blockIdx.x * nw + wave; i < P.n; i += gridDim.x * nw)
                        if (lane < 3) A.rows[0][3 * (size_t)i + lane] = A.rows[1][3 * (size_t)i + lane];
                        else if (lane == 3 && A.qcert[0]) A.qcert[0][i] = A.qcert[1][i];
                }
            }
            return;
        }
    }
}

}  // namespace
}  // namespace sp

#ifdef SP_OPT_TIMING
extern "C" int sp_internal_opt_debug(unsigned long long* out384) {
    return hipMemcpyFromSymbol(out384, HIP_SYMBOL(sp::g_sp_dbg), 24 * 16 * 8) == hipSuccess ? 0 : 3;
}
extern "C" int sp_internal_opt_debug_wg(unsigned long long* out192) {
    return hipMemcpyFromSymbol(out192, HIP_SYMBOL(sp::g_sp_wg), 24 * 8 * 8) == hipSuccess ? 0 : 3;
}
#endif
extern "C" int sp_gicp_align_optimize(const sp_gicp_target* target, const sp_gicp_source* source, float* transT_device,
                                     const sp_factor_params* params, const sp_opt_params* opt, const float* robust_scales,
                                     int n_levels, sp_align_result* result_device, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    using namespace sp;
    hipStream_t st = as_stream(stream);
    if (!target || !source || !params || !opt || !transT_device || !result_device || !robust_scales) return SP_ERR_INVALID_ARGUMENT;
    if (const int rc = check_opt_args("sp_gicp_align_optimize", opt, n_levels, "the result is the initial guess"); rc != SP_OK) return rc;
    if (const int rc = check_prepared_reg(target, params); rc != SP_OK) return rc;
    const size_t n = source->n;
    if (n == 0) {
        sp_set_error("[sp_gicp_align_optimize] empty source (Registration::align returns the initial guess)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (const int rc = check_workspace(workspace, workspace_bytes, n); rc != SP_OK) return rc;
    if (source->opt_persistent == 0) {
        sp_set_error("[sp_gicp_align_optimize] not available: persistent launches are switched off for this source "
                     "(sp_gicp_source_set_persistent)");
        return SP_ERR_RUNTIME;
    }
    // workgroups of 256 lanes while they all fit the device one per compute unit (64 K points), of 1024 beyond
    const bool small = n <= (size_t)256 * 256;
    const unsigned block = small ? 256u : (unsigned)kAlignBlock;
    const bool fast = source_fast_nn(source);
    const bool waveq = fast && ((source->opt_wave_query == 1 && n <= kWaveQueryMax) || (source->opt_wave_query == 2 && n <= kWaveQueryForcedMax));
    // (wave per point: four waves a workgroup, each alone on its SIMD with 256 registers, up to two points a wave; beyond, sixteen
    // waves a workgroup: a wave then walks through its points one after the other and the other waves of its SIMD hide its round
    // trips — 212 against 404 us per iteration on the reference's bundled scans)
    const unsigned wq_block = n <= kWaveQueryMax ? 256u : (unsigned)kAlignBlock;
    const unsigned wq_waves = wq_block / kWave;
    const unsigned grid = std::min<unsigned>((unsigned)(waveq ? (n + wq_waves - 1) / wq_waves : (n + block - 1) / block), (unsigned)kAlignMaxBlocks);
    PersistGuard* const guard = persist_acquire(st, grid);
    if (!guard) {
        sp_set_error("[sp_gicp_align_optimize] not available now: the launch cannot be resident (grid larger than the device, stream "
                     "capturing, or another stream's persistent launch still running)");
        return SP_ERR_RUNTIME;
    }
    struct Release {
        PersistGuard* g; hipStream_t st;
        ~Release() { persist_release(g, st); }
    } release{guard, st};
    OptArgs A;
    float* const rows = static_cast<float*>(workspace);
    A.part[0] = rows;
    A.part[1] = rows + (size_t)kAlignMaxBlocks * kPartial;
    A.tickets = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + kTicketOffsetBytes);
    A.trows[0] = source->opt_rows;
    A.trows[1] = source->opt_rows + (size_t)kAlignMaxBlocks * 32;
    A.rows[0] = source->ccache;
    A.rows[1] = source->ccache2;
    // (the margin certificates: with the reuse of correspondences on, for sources the wave-per-point form serves)
    const bool margin_certs = waveq && source->opt_reuse != 0 && source->qcert != nullptr && n <= source->qcert_points;
    A.qcert[0] = margin_certs ? source->qcert : nullptr;
    A.qcert[1] = margin_certs ? source->qcert2 : nullptr;
    A.qcert_trusted = (margin_certs && source->qcert_valid && source->cache_valid) ? 1 : 0;
    // (trial steps that also linearise: the wave-per-point launches of 256-lane workgroups, where a step is a hand-off between
    // hundreds of workgroups around two microseconds of work)
    A.fuse = (waveq && wq_block == 256u && source->ccache2 != nullptr && source->opt_fuse_trials && (!margin_certs || source->qcert2 != nullptr)) ? 1 : 0;
    A.tag_base = 0;
    if (grid > 1 && waveq) {
        // a row's tag is (epoch of the launch, step): rows left by earlier launches never match, so nothing is zeroed per launch —
        // only when the 12-bit epoch wraps (the buffer is zero when the source is created)
        if (++source->opt_epoch >= 4096u) {
            if (zero_async(source->opt_rows, kOptRowsBytes, st) != SP_OK) return SP_ERR_HIP;
            source->opt_epoch = 1;
        }
        A.tag_base = source->opt_epoch << 20;
    } else if (grid > 1 && zero_async(A.tickets, kTicketShards * kTicketStride * sizeof(unsigned), st) != SP_OK) return SP_ERR_HIP;
    target->note(st);
    FusedParams P = make_fused_params(target, source, params, transT_device, 1, nullptr, nullptr);
    A.T_init = transT_device;
    A.T_out = transT_device;
    A.opt = *opt;
    fill_level_scales(A.scales, robust_scales, n_levels);
    A.n_levels = n_levels;
    A.reuse = (source->opt_reuse && P.ccache != nullptr) ? 1 : 0;
    A.result = result_device;
    A.budget = 50ull * 100000ull;  // 50 ms of wall_clock64 (100 MHz) per wait
    if (P.ccache == nullptr) {  // (a target without certificates has no cache rows: the trial steps read them)
        sp_set_error("[sp_gicp_align_optimize] the prepared target has no reuse certificates");
        return SP_ERR_INVALID_ARGUMENT;
    }
    const int rc = with_variant(params->robust_type, fast, params->reg_type == SP_REG_POINT_TO_DISTRIBUTION,
                                [&](auto L, auto FAST_NN, auto P2D) {
        constexpr int loss = L;
        constexpr bool fast_nn = FAST_NN, p2d = P2D;
        return with_bool<false>((waveq ? wq_block : block) == 256u, [&](auto SMALL) {
            constexpr int B = decltype(SMALL)::value ? 256 : kAlignBlock;
            if constexpr (fast_nn) {  // (a wave per point exists with the fast search only: waveq implies fast)
                if (waveq) {
                    gicp_optimize_kernel<loss, true, p2d, B, true><<<grid, B, 0, st>>>(P, A);
                    return SP_OK;
                }
            }
            gicp_optimize_kernel<loss, fast_nn, p2d, B><<<grid, B, 0, st>>>(P, A);
            return SP_OK;
        });
    });
    if (rc != SP_OK) return rc;
    source->cache_valid = true;
    source->qcert_valid = margin_certs;
    return launch_status();
}
