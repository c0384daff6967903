// The optimiser of Registration::align as ONE state machine (replaces registration.hpp:201-276, 803-828, 830-895, 897-964 and
// pipeline/robust.hpp:100-111): which trial to evaluate, when to take it, how lambda / the trust radius move, when an outer
// iteration, a level and the alignment end. Host-and-device code over one plain struct, compiled with -ffp-contract=off on both
// sides: one lane of the device-resident launch runs it on LDS (registration_opt.hip), the host stepper of the C ABI
// (sp_opt_stepper_*, opt_stepper.hip) runs it for the host-driven loops of the C++ facade and the Python package. The update
// rules live here and nowhere else.
#ifndef SP_OPTIMIZER_H
#define SP_OPTIMIZER_H

#include <string>

#include "registration_device.h"

namespace sp {
namespace {

// PHASE_FUSED (wave-per-point launches of 256-lane workgroups): a trial step that ALSO linearises at the trial pose, into the
// other set of cache rows — accepted trials are the rule, and the linearisation of the next outer iteration is then already
// there: an outer iteration costs one step (one hand-off between the workgroups) instead of two.
enum { PHASE_LIN = 0, PHASE_TRIAL = 1, PHASE_FUSED = 2 };

struct OptCtl {  // the optimiser's state between steps
    int phase;
    int done;             // 0 go on, 1 finished, 2 a wait ran out
    int level, iter, inner;
    int cache_valid;
    float lambda, radius;
    float cur_error, last_error;
    float predicted, step_norm;  // dog-leg step in flight
    int conv_ok;          // trial step: success ? is_converged(delta) : false   (registration.hpp:843-847)
    int conv_any;         // trial step: is_converged(delta)                      (:867, :878, :951)
    int converged;
    float res_error;
    unsigned res_inlier, res_iterations;
    unsigned n_lin, n_trial, searched, log_n;
    int took;             // the latest trial's pose became the pose
    int spec_level;       // PHASE_FUSED: the level whose robust scale the speculative linearisation uses
    int cur;              // which set of cache rows holds the correspondences of the latest linearisation (0: the source's own)
};

SP_HD float clampf(float v, float lo, float hi) { return v < lo ? lo : (hi < v ? hi : v); }  // std::clamp

SP_HD bool is_converged6(const float* d, float crit_rot, float crit_trans) {  // registration.hpp:407-410
    const float nr = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const float nt = sqrtf(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
    return nr < crit_rot && nt < crit_trans;
}

struct OptState {
    float sT[16];      // current pose (result.T)
    float sTt[16];     // trial pose
    float sTlin[16];   // pose of the latest linearisation
    sp_linearized slin;  // system of the latest linearisation
    float sdelta[8];
    LdltScratch ldlt_ws;
    OptCtl ctl;
    // what the state machine reads of its caller's arguments (on the device it is a real function: arguments passed by reference
    // would have to live in scratch memory for the whole kernel)
    sp_opt_params opt;
    int n_levels, reuse;
    sp_align_result* result;  // where the log entries go
};

SP_HD void opt_start(OptCtl& c, const sp_opt_params& o, int cache_valid) {
    c.phase = PHASE_LIN; c.done = 0; c.level = 0; c.iter = 0; c.inner = 0;
    c.cache_valid = cache_valid;
    c.lambda = o.lm_init_lambda; c.radius = o.dl_initial_radius;
    c.cur_error = 0.0f; c.last_error = FLT_MAX; c.predicted = 0.0f; c.step_norm = 0.0f;
    c.conv_ok = 0; c.conv_any = 0; c.converged = 0;
    c.res_error = FLT_MAX; c.res_inlier = 0; c.res_iterations = 0;
    c.n_lin = 0; c.n_trial = 0; c.searched = 0; c.log_n = 0;
    c.took = 0; c.spec_level = 0; c.cur = 0;
}

// One LM trial: delta = LDLT(H + lambda I).solve(-b), T_trial = T exp(delta)   (registration.hpp:841-848)
SP_HD void lm_try(OptState& S) {
    const sp_opt_params& o = S.opt;
#pragma unroll
    for (int i = 0; i < 16; ++i) S.sTt[i] = S.sT[i];
    gn_update_impl(&S.slin, S.sTt, S.ctl.lambda, o.crit_rotation, o.crit_translation, S.sdelta, false, S.ldlt_ws);
    S.ctl.conv_ok = S.sdelta[6] > 0.5f ? 1 : 0;
    S.ctl.conv_any = is_converged6(S.sdelta, o.crit_rotation, o.crit_translation) ? 1 : 0;
    S.ctl.phase = PHASE_TRIAL;
}

// An outer iteration has ended (`accepted`: sp_opt_log_entry::accepted): log it; converged or the last iteration ends the
// level (registration.hpp:266-268); after the last level the alignment is done.
SP_HD void end_outer(OptState& S, int accepted, unsigned trials, bool publish) {
    OptCtl& c = S.ctl;
    const sp_opt_params& o = S.opt;
    c.res_iterations = (unsigned)c.iter;
    if (publish && c.log_n < (unsigned)SP_OPT_LOG_ENTRIES) {
        sp_opt_log_entry e;
        e.level = (uint16_t)c.level; e.iteration = (uint16_t)c.iter; e.trials = (uint16_t)trials; e.accepted = (uint16_t)accepted;
        e.damping = o.method == SP_OPT_POWELL_DOGLEG ? c.radius : c.lambda;
        e.error = c.res_error;
        S.result->log[c.log_n] = e;
    }
    ++c.log_n;
    if (!c.converged && c.iter + 1 < o.max_iterations) {
        ++c.iter;
        c.phase = PHASE_LIN;
        c.cache_valid = S.reuse;
        return;
    }
    if (c.level + 1 < S.n_levels) {  // the next robust scale: a fresh align() from this pose (pipeline/robust.hpp:100-111)
        ++c.level;
        c.iter = 0;
        c.lambda = o.lm_init_lambda;
        c.radius = o.dl_initial_radius;
        c.converged = 0;
        c.res_error = FLT_MAX;  // RegistrationResult's defaults (result.hpp:12-28)
        c.res_inlier = 0;
        c.res_iterations = 0;
        c.phase = PHASE_LIN;
        c.cache_valid = S.reuse;  // certificates prove every reused correspondence: the same neighbours as a fresh search
        return;
    }
    c.done = 1;
}

// After a linearisation at S.sT whose reduced system the caller has put into S.slin.
SP_HD void opt_after_linearize(OptState& S, bool publish) {
    OptCtl& c = S.ctl;
#pragma unroll
    for (int i = 0; i < 16; ++i) S.sTlin[i] = S.sT[i];
    const sp_opt_params& o = S.opt;
    if (o.method == SP_OPT_GAUSS_NEWTON) {  // registration.hpp:803-828
        gn_update_impl(&S.slin, S.sT, o.gn_lambda, o.crit_rotation, o.crit_translation, S.sdelta, false, S.ldlt_ws);
        c.converged = S.sdelta[6] > 0.5f ? 1 : 0;
        c.res_error = S.slin.error;
        c.res_inlier = S.slin.inlier;
        end_outer(S, 1, 0, publish);
    } else if (o.method == SP_OPT_LEVENBERG_MARQUARDT) {  // :830-895
        c.cur_error = S.slin.error;
        c.last_error = FLT_MAX;
        c.inner = 0;
        if (o.lm_max_inner_iterations <= 0) end_outer(S, 0, 0, publish);  // (no trial: result.converged stays false)
        else lm_try(S);
    } else {  // :897-964
        c.res_error = S.slin.error;
        c.res_inlier = S.slin.inlier;
        c.cur_error = S.slin.error;
        c.radius = clampf(c.radius, o.dl_min_radius, o.dl_max_radius);
        const DoglegStep6 dl = dogleg_step6(S.slin.H, S.slin.b, c.radius, S.ldlt_ws);
        if (dl.predicted_reduction <= 0.0f) {
            c.radius = clampf(c.radius * o.dl_gamma_decrease, o.dl_min_radius, o.dl_max_radius);
            end_outer(S, 0, 0, publish);
        } else {
            const Rigid upd = rigid_mul(load_rigid_colmajor(S.sT), se3_exp(dl.p));
            store_rigid_colmajor(upd, S.sTt);
            c.conv_any = is_converged6(dl.p, o.crit_rotation, o.crit_translation) ? 1 : 0;
            c.predicted = dl.predicted_reduction;
            c.step_norm = dl.step_norm;
            c.phase = PHASE_TRIAL;
        }
    }
}

// After a trial: the robust error and the inlier count at S.sTt over the correspondences frozen at S.sTlin. Returns the gain
// ratio rho of a dog-leg trial (0 for LM), for callers that print it.
SP_HD float opt_after_trial(OptState& S, float new_error, unsigned inl, bool publish) {
    OptCtl& c = S.ctl;
    const sp_opt_params& o = S.opt;
    ++c.n_trial;
    c.took = 0;
    auto take = [&] {
#pragma unroll
        for (int i = 0; i < 16; ++i) S.sT[i] = S.sTt[i];
        c.res_error = new_error;
        c.res_inlier = inl;
        c.took = 1;
    };
    float rho = 0.0f;
    if (o.method == SP_OPT_LEVENBERG_MARQUARDT) {
        const unsigned tries = (unsigned)c.inner + 1u;
        if (new_error <= c.cur_error) {  // :866-876
            c.converged = c.conv_any;
            take();
            c.lambda = clampf(c.lambda / o.lm_lambda_factor, o.lm_min_lambda, o.lm_max_lambda);
            end_outer(S, 1, tries, publish);
        } else if (fabsf(new_error - c.last_error) <= 1e-6f) {  // :877-884
            c.converged = c.conv_any;
            take();
            end_outer(S, 2, tries, publish);
        } else {  // :885-889
            c.lambda = clampf(c.lambda * o.lm_lambda_factor, o.lm_min_lambda, o.lm_max_lambda);
            c.last_error = new_error;
            ++c.inner;
            if (c.inner < o.lm_max_inner_iterations) {
                lm_try(S);
            } else {
                c.converged = c.conv_ok;  // what the last trial left in result.converged (:843-847)
                end_outer(S, 0, tries, publish);
            }
        }
    } else {  // dog-leg (:936-962)
        rho = (c.cur_error - new_error) / c.predicted;
        if (rho < o.dl_eta1) {
            c.radius = clampf(c.radius * o.dl_gamma_decrease, o.dl_min_radius, o.dl_max_radius);
            end_outer(S, 0, 1, publish);
        } else {
            c.converged = c.conv_any;
            take();
            if (rho > o.dl_eta2 && c.step_norm >= c.radius * 0.99f)
                c.radius = clampf(c.radius * o.dl_gamma_increase, o.dl_min_radius, o.dl_max_radius);
            end_outer(S, 1, 1, publish);
        }
    }
    return rho;
}

// RegistrationResult of the latest level + the linearisation pose + counters: the scalar fields of the result block.
SP_HD void opt_result_scalars(const OptState& S, sp_align_result* r) {
    const OptCtl& c = S.ctl;
    r->error = c.res_error;
    r->error_raw = S.slin.error;
    r->inlier = c.res_inlier;
    r->iterations = c.res_iterations;
    r->converged = (unsigned)c.converged;
    r->status = 0u;
    r->linearizations = c.n_lin;
    r->trials = c.n_trial;
    r->searched = c.searched;
    r->damping = S.opt.method == SP_OPT_POWELL_DOGLEG ? c.radius : c.lambda;
    r->log_entries = c.log_n < (unsigned)SP_OPT_LOG_ENTRIES ? c.log_n : (unsigned)SP_OPT_LOG_ENTRIES;
    r->pad[1] = r->pad[2] = 0u;  // (pad[0]: the done flag of the device launch, stored last by its caller)
}

// ---- host: what every entry point that takes the optimiser's arguments checks, under the caller's own name
inline int invalid(const char* msg) {
    sp_set_error(msg);
    return SP_ERR_INVALID_ARGUMENT;
}
// `zero_iterations`: what the caller's result is without an iteration, the tail of the max_iterations message.
inline int check_opt_args(const char* fn, const sp_opt_params* opt, int n_levels, const char* zero_iterations) {
    const std::string at = std::string("[") + fn + "] ";
    if (n_levels < 1 || n_levels > SP_OPT_MAX_LEVELS) return invalid((at + "n_levels must be in 1..SP_OPT_MAX_LEVELS").c_str());
    if (opt->method != SP_OPT_GAUSS_NEWTON && opt->method != SP_OPT_LEVENBERG_MARQUARDT && opt->method != SP_OPT_POWELL_DOGLEG)
        return invalid((at + "unknown optimization method").c_str());
    if (opt->max_iterations < 1 || opt->max_iterations > 65535)
        return invalid((at + "max_iterations must be in 1..65535 (0 iterations: " + zero_iterations + ")").c_str());
    return SP_OK;
}
// One robust scale per annealing level; the levels past n_levels repeat the last one.
inline void fill_level_scales(float (&dst)[SP_OPT_MAX_LEVELS], const float* robust_scales, int n_levels) {
    for (int l = 0; l < SP_OPT_MAX_LEVELS; ++l) dst[l] = robust_scales[l < n_levels ? l : n_levels - 1];
}

}  // namespace
}  // namespace sp
#endif
