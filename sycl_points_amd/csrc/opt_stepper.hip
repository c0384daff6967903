// The optimiser's state machine (sp_optimizer.h) for a host-driven loop: the caller linearises and evaluates trials wherever it
// likes and the stepper takes every decision of Registration::align (registration.hpp:201-276, 803-964) and of the annealing
// levels around it (pipeline/robust.hpp:100-111) with the code one lane of sp_gicp_align_optimize's launch runs. Host memory only.
#include <new>

#include "sp_optimizer.h"

struct sp_opt_stepper {
    sp::OptState S;
    sp_align_result res;  // the log entries as they are written
    float scales[SP_OPT_MAX_LEVELS];
};

extern "C" int sp_opt_stepper_create(const sp_opt_params* opt, const float* T_init16, const float* robust_scales, int n_levels,
                                     sp_opt_stepper** out) {
    if (!opt || !T_init16 || !robust_scales || !out) return SP_ERR_INVALID_ARGUMENT;
    if (n_levels < 1 || n_levels > SP_OPT_MAX_LEVELS) {
        sp_set_error("[sp_opt_stepper_create] n_levels must be in 1..SP_OPT_MAX_LEVELS");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (opt->method != SP_OPT_GAUSS_NEWTON && opt->method != SP_OPT_LEVENBERG_MARQUARDT && opt->method != SP_OPT_POWELL_DOGLEG) {
        sp_set_error("[sp_opt_stepper_create] unknown optimization method");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (opt->max_iterations < 0) {
        sp_set_error("[sp_opt_stepper_create] max_iterations must not be negative");
        return SP_ERR_INVALID_ARGUMENT;
    }
    sp_opt_stepper* const s = new (std::nothrow) sp_opt_stepper();  // (zeroed)
    if (!s) return SP_ERR_RUNTIME;
    for (int i = 0; i < 16; ++i) s->S.sT[i] = s->S.sTt[i] = s->S.sTlin[i] = T_init16[i];
    sp::opt_start(s->S.ctl, *opt, 0);
    s->S.opt = *opt;
    s->S.n_levels = n_levels;
    s->S.result = &s->res;
    for (int l = 0; l < n_levels; ++l) s->scales[l] = robust_scales[l];
    if (opt->max_iterations == 0) s->S.ctl.done = 1;  // the reference's loop does not run (:227): the result is the initial guess
    *out = s;
    return SP_OK;
}

extern "C" void sp_opt_stepper_destroy(sp_opt_stepper* s) { delete s; }

extern "C" int sp_opt_stepper_next(const sp_opt_stepper* s, sp_opt_request* out) {
    if (!s || !out) return SP_ERR_INVALID_ARGUMENT;
    const sp::OptCtl& c = s->S.ctl;
    out->want = c.done ? SP_OPT_WANT_DONE : c.phase == sp::PHASE_LIN ? SP_OPT_WANT_LINEARIZE : SP_OPT_WANT_TRIAL;
    out->level = c.level;
    out->iteration = c.iter;
    out->robust_scale = s->scales[c.level];
    const float* const T = out->want == SP_OPT_WANT_TRIAL ? s->S.sTt : s->S.sT;
    for (int i = 0; i < 16; ++i) { out->T[i] = T[i]; out->T_lin[i] = s->S.sTlin[i]; }
    out->damping = s->S.opt.method == SP_OPT_POWELL_DOGLEG ? c.radius : c.lambda;
    return SP_OK;
}

extern "C" int sp_opt_stepper_linearized(sp_opt_stepper* s, const sp_linearized* lin_host) {
    if (!s || !lin_host) return SP_ERR_INVALID_ARGUMENT;
    if (s->S.ctl.done || s->S.ctl.phase != sp::PHASE_LIN) {
        sp_set_error("[sp_opt_stepper_linearized] no linearisation was asked for (sp_opt_stepper_next)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    s->S.slin = *lin_host;
    ++s->S.ctl.n_lin;
    sp::opt_after_linearize(s->S, true);
    return SP_OK;
}

extern "C" int sp_opt_stepper_trial(sp_opt_stepper* s, float error, uint32_t inlier, float* rho_out) {
    if (!s) return SP_ERR_INVALID_ARGUMENT;
    if (s->S.ctl.done || s->S.ctl.phase != sp::PHASE_TRIAL) {
        sp_set_error("[sp_opt_stepper_trial] no trial was asked for (sp_opt_stepper_next)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    const float rho = sp::opt_after_trial(s->S, error, inlier, true);
    if (rho_out) *rho_out = rho;
    return SP_OK;
}

extern "C" int sp_opt_stepper_result(const sp_opt_stepper* s, sp_align_result* out) {
    if (!s || !out) return SP_ERR_INVALID_ARGUMENT;
    *out = s->res;
    for (int i = 0; i < 16; ++i) { out->T[i] = s->S.sT[i]; out->T_lin[i] = s->S.sTlin[i]; }
    for (int i = 0; i < 36; ++i) out->H[i] = s->S.slin.H[i];
    for (int i = 0; i < 6; ++i) out->b[i] = s->S.slin.b[i];
    sp::opt_result_scalars(s->S, out);
    out->pad[0] = s->S.ctl.done ? (uint32_t)SP_ALIGN_RESULT_DONE : 0u;
    return SP_OK;
}
