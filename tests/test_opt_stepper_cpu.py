"""The optimiser's state machine without a GPU (csrc/sp_optimizer.h through the host stepper of the C ABI, sp_opt_stepper_*):
the code one lane of sp_gicp_align_optimize's launch runs, driven here with the ORACLE as the device — brute-force nearest
neighbours + the oracle's K11 for a linearisation, its K12 for a trial — and compared with the oracle's own align() on the same
clouds (the inputs, initial guess and cases of tests/test_gpu_optimize.py). Both sides then consume the same sums, and the
solver under the state machine is pinned bit for bit against the oracle's (tests/test_cabi.py), so Gauss-Newton and
Levenberg-Marquardt without pose terms have to agree in every bit; where a piece is not bit-pinned (the dog-leg step, NL-Reg,
the MAP prior) the rule of the GPU test applies unchanged."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_optimize import CASES, check_against_oracle, inputs, oracle_params

T0_TWIST = [0.01, -0.005, 0.02, 0.05, -0.04, 0.03]


@pytest.fixture(scope="module")
def sp():
    from sycl_points_amd import _lib

    _lib.build()  # hipcc cross-compiles without a GPU; nothing happens when the library is current
    import sycl_points_amd.api as api

    return api


@pytest.fixture(scope="module")
def clouds(orc):
    return inputs(orc, 900, 8.0)


def colmajor(T):
    return np.ascontiguousarray(np.asarray(T, np.float32).T).reshape(-1)


def floats(*v):
    return (C.c_float * len(v))(*v)


def run_stepper(sp, orc, clouds, case, T0, scales, max_iterations, dreg=None, prior=None):
    """The ask-and-serve loop of the library's host loops with the oracle's kernels. dreg: DegenerateRegParams; prior:
    MapPriorState. Returns the RegistrationResult of the stepper's sp_align_result and the dog-leg gain ratios it reported."""
    src, scov, tgt, tcov = clouds[:4]
    L, lib = sp._lib.lib(), sp._lib
    p = sp.RegistrationParams(reg_type=case["reg_type"], robust_type=case["loss"], robust_default_scale=case["scale"],
                              optimization_method=case["opt"], max_iterations=max_iterations)
    op, h, req, r = sp.Registration(p).opt_params(), C.c_void_p(), lib.OptRequest(), lib.AlignResult()
    T0c, rhos = colmajor(T0), []
    sp.check(L.sp_opt_stepper_create(C.byref(op), T0c.ctypes.data, floats(*scales), len(scales), C.byref(h)))
    try:
        nn = lin_T = None
        while True:
            sp.check(L.sp_opt_stepper_next(h, C.byref(req)))
            if req.want == lib.OPT_WANT_DONE:
                break
            assert req.robust_scale == np.float32(scales[req.level])
            Tc = np.array(req.T, np.float32)
            T = Tc.reshape(4, 4).T
            if req.want == lib.OPT_WANT_LINEARIZE:
                nn, lin_T = orc.knn_bruteforce(orc.transform_points(src, T), tgt, 1), Tc
                o = orc.gicp_linearize(src, scov, tgt, tcov, None, nn[0], nn[1], T, 2.0, case["reg_type"], case["loss"],
                                       req.robust_scale)
                lr = lib.Linearized()
                lr.H[:] = o["H"].reshape(-1).tolist()
                lr.b[:] = o["b"].tolist()
                lr.error, lr.inlier = o["error"], o["inlier"]
                if dreg is not None:  # registration.hpp:249-250
                    sp.check(L.sp_degenerate_regularize_host(C.byref(dreg), lr.H, lr.b, lr.inlier, Tc.ctypes.data, T0c.ctypes.data))
                if prior is not None:  # registration.hpp:253
                    err = C.c_float(lr.error)
                    L.sp_map_prior_apply_host(C.byref(prior), Tc.ctypes.data, lr.H, lr.b, C.byref(err))
                    lr.error = err.value
                sp.check(L.sp_opt_stepper_linearized(h, C.byref(lr)))
            else:
                assert np.array_equal(np.array(req.T_lin, np.float32), lin_T)  # the frozen correspondences are the latest ones
                e, inl = orc.gicp_error(src, scov, tgt, tcov, None, nn[0], nn[1], T, 2.0, case["reg_type"], case["loss"],
                                        req.robust_scale)
                e = np.float32(e)
                if prior is not None:  # registration.hpp:854, :933
                    e = np.float32(e + np.float32(L.sp_map_prior_apply_host(C.byref(prior), Tc.ctypes.data, None, None, None)))
                rho = C.c_float(-1.0)
                sp.check(L.sp_opt_stepper_trial(h, C.c_float(e), inl, C.byref(rho)))
                rhos.append(rho.value)
        sp.check(L.sp_opt_stepper_result(h, C.byref(r)))
    finally:
        L.sp_opt_stepper_destroy(h)
    assert r.pad[0] == 0x600DF00D and r.status == 0 and r.searched == 0
    return sp.Registration._result_from_align_result(r), rhos


def assert_bit_equal(res, ref, case):
    """Pose, counters, flags and the per-iteration (trials, accepted, damping, error) sequence: every bit."""
    f32 = np.float32
    assert np.array_equal(res.T, ref["T"]), (case, np.abs(res.T - ref["T"]).max())
    assert (res.iterations, res.converged, res.inlier) == (ref["iterations"], ref["converged"], ref["inlier"]), case
    assert f32(res.error) == f32(ref["error"]), case
    got = [(e["trials"], e["accepted"], f32(e["damping"]), f32(e["error"])) for e in res.log]
    want = [(s["trials"], s["accepted"], f32(s["damping"]), f32(s["error"])) for s in ref["steps"]]
    assert got == want, (case, got, want)
    assert res.linearizations == len(want) and res.trials == sum(s["trials"] for s in ref["steps"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['opt']}-{c['reg_type']}-{c['loss']}")
def test_stepper_with_the_oracle_as_device_matches_oracle_align(sp, orc, clouds, case):
    src, scov, tgt, tcov, _ = clouds
    T0 = orc.se3_exp(T0_TWIST)
    ref = orc.registration_align(oracle_params(case, max_iterations=25), src, scov, tgt, tcov, init_T=T0, nn_mode="bruteforce",
                                 steps=True)
    res, rhos = run_stepper(sp, orc, clouds, case, T0, [case["scale"]], 25)
    check_against_oracle(res, ref, case)
    if case["opt"] != "DOGLEG":  # same sums in, bit-pinned solver: nothing may differ
        assert_bit_equal(res, ref, case)
        assert not any(rhos)
    else:
        assert len(rhos) == res.trials and all(np.isfinite(rhos)) and rhos[0] > 0.25  # (the first step is accepted: rho >= eta1)


@pytest.mark.parametrize("opt", ["LM", "DOGLEG", "GN"])
def test_stepper_annealing_levels_match_oracle(sp, orc, opt):
    """Three levels (Geman-McClure, 10 -> 5 -> 2.5, at most 10 iterations each: test_annealing_levels_in_one_launch) in one stepper."""
    cl = inputs(orc, 1000, 8.0, seed=99)
    case = dict(opt=opt, reg_type="GICP", loss="GEMAN_MCCLURE", scale=10.0)
    ref = orc.registration_align(oracle_params(case, max_iterations=10, auto_scale=1, auto_scaling_iter=3, init_scale=10.0,
                                               min_scale=2.5), cl[0], cl[1], cl[2], cl[3], nn_mode="bruteforce", steps=True)
    scales = [float(s) for s in orc.robust_annealing_scales("GEMAN_MCCLURE", True, 10.0, 10.0, 2.5, 3)]
    res, _ = run_stepper(sp, orc, cl, case, np.eye(4, dtype=np.float32), scales, 10)
    check_against_oracle(res, ref, case, levels=3)
    if opt != "DOGLEG":
        assert_bit_equal(res, ref, case)


@pytest.mark.parametrize("opt", ["LM", "DOGLEG"])
@pytest.mark.parametrize("term", ["NL_REG", "MAP_PRIOR"])
def test_stepper_with_host_side_pose_terms_matches_oracle(sp, orc, clouds, opt, term):
    """Degenerate regularisation / the MAP prior applied to the reduced system by the caller (sp_degenerate_regularize_host,
    sp_map_prior_apply_host: agree with the oracle's to ~1e-5, not bit for bit), the prior's error added to every trial."""
    src, scov, tgt, tcov, _ = clouds
    lib, L = sp._lib, sp._lib.lib()
    case = dict(opt=opt, reg_type="GICP", loss="NONE", scale=10.0)
    T0 = orc.se3_exp(T0_TWIST)
    prev = orc.registration_align(oracle_params(dict(case, opt="GN"), max_iterations=3), src, scov, tgt, tcov, nn_mode="bruteforce")
    kw, dreg, prior = {}, None, None
    if term == "NL_REG":  # thresholds above the smallest eigenvalue of each block: at least one axis of each penalised
        thr_rot = float(np.linalg.eigvalsh(prev["H_raw"][:3, :3].astype(np.float64))[0] / prev["inlier"]) * 1.5
        thr_tr = float(np.linalg.eigvalsh(prev["H_raw"][3:, 3:].astype(np.float64))[0] / prev["inlier"]) * 1.5
        kw = dict(dr_type=1, dr_rot_threshold=thr_rot, dr_trans_threshold=thr_tr, dr_base_factor=0.5)
        dreg = lib.DegenerateRegParams(1, thr_rot, thr_tr, 0.5)
    else:
        T_pred = orc.isometry_mul(prev["T"], orc.se3_exp([0.002, -0.001, 0.001, 0.01, 0.0, -0.005]))
        has, Om, Tinv = orc.map_prior_update(prev["H_raw"], prev["error_raw"], prev["inlier"], prev["T"], T_pred)
        assert has
        kw = dict(map_prior=(Om, Tinv))
        prior, mp = lib.MapPriorState(), lib.MapPriorParams(1, 1.0, 1.0, 3.16e-2, 1e-2)
        Hc = np.ascontiguousarray(prev["H_raw"])
        assert L.sp_map_prior_update_host(C.byref(mp), Hc.ctypes.data, prev["error_raw"], prev["inlier"],
                                          colmajor(prev["T"]).ctypes.data, colmajor(T_pred).ctypes.data, C.byref(prior)) == 0
        assert prior.has_prior == 1
    ref = orc.registration_align(oracle_params(case, max_iterations=25, **kw), src, scov, tgt, tcov, init_T=T0,
                                 nn_mode="bruteforce", steps=True)
    plain = orc.registration_align(oracle_params(case, max_iterations=25), src, scov, tgt, tcov, init_T=T0, nn_mode="bruteforce")
    assert not np.array_equal(ref["H"], plain["H"]), "the term must be in the system"
    res, _ = run_stepper(sp, orc, clouds, case, T0, [case["scale"]], 25, dreg=dreg, prior=prior)
    check_against_oracle(res, ref, case)
    assert np.abs(res.H - ref["H"]).max() <= 5e-5 * np.abs(ref["H"]).max()


def test_stepper_corners_follow_the_reference(sp, orc):
    """max_iterations 0: the loop does not run, the result is the initial guess with RegistrationResult's defaults
    (registration.hpp:227). LM without inner iterations: every outer iteration linearises, tries nothing, converged stays false
    (:842). An accepted LM trial after a failed solve (delta = 0): converged is is_converged(delta), true (:866) — the solver's
    flag (:848, false) only stands when no trial is accepted."""
    lib, L = sp._lib, sp._lib.lib()
    T0 = colmajor(orc.se3_exp(T0_TWIST))

    def start(**kw):
        op, h = sp.Registration(sp.RegistrationParams(**kw)).opt_params(), C.c_void_p()
        sp.check(L.sp_opt_stepper_create(C.byref(op), T0.ctypes.data, floats(10.0), 1, C.byref(h)))
        return h

    def state(h):
        req, r = lib.OptRequest(), lib.AlignResult()
        sp.check(L.sp_opt_stepper_next(h, C.byref(req)))
        sp.check(L.sp_opt_stepper_result(h, C.byref(r)))
        return req, r

    def system(diag, off45=0.0):
        lin = lib.Linearized()
        for i in range(6):
            lin.H[i * 7] = diag[i]
            lin.b[i] = 0.5
        lin.H[4 * 6 + 5] = lin.H[5 * 6 + 4] = off45
        lin.error, lin.inlier = 3.0, 7
        return lin

    h = start(optimization_method="LM", max_iterations=0)
    req, r = state(h)
    assert req.want == lib.OPT_WANT_DONE and np.array_equal(np.array(r.T, np.float32), T0)
    assert (r.iterations, r.converged, r.inlier, r.log_entries) == (0, 0, 0, 0) and r.error == np.finfo(np.float32).max
    L.sp_opt_stepper_destroy(h)

    h = start(optimization_method="LM", max_iterations=100000, lm_max_inner_iterations=0)  # (no 16-bit limit on the host)
    for it in range(3):
        req, _ = state(h)
        assert req.want == lib.OPT_WANT_LINEARIZE and req.iteration == it and np.array_equal(np.array(req.T, np.float32), T0)
        sp.check(L.sp_opt_stepper_linearized(h, C.byref(system([4.0] * 6))))
    req, r = state(h)
    assert req.want == lib.OPT_WANT_LINEARIZE and (r.iterations, r.converged, r.trials, r.linearizations) == (2, 0, 0, 3)
    assert [(e.trials, e.accepted) for e in r.log[:r.log_entries]] == [(0, 0)] * 3
    L.sp_opt_stepper_destroy(h)

    # H + lambda I (lambda = 1) = diag(5, 5, 5, 5) + [[0, 1], [1, 0]]: the fifth pivot is zero under a non-zero column
    bad = system([4.0, 4.0, 4.0, 4.0, -1.0, -1.0], 1.0)
    d8, Tt = np.zeros(8, np.float32), T0.copy()
    L.sp_gn_update_host(C.byref(bad), Tt.ctypes.data, 1.0, 1e-3, 1e-3, d8.ctypes.data)
    assert d8[7] == 0.0 and not d8[:6].any(), "this system must fail the solve for the case to mean anything"
    h = start(optimization_method="LM", max_iterations=5)
    sp.check(L.sp_opt_stepper_linearized(h, C.byref(bad)))
    req, _ = state(h)
    assert req.want == lib.OPT_WANT_TRIAL and np.array_equal(np.array(req.T, np.float32), T0)  # delta = 0
    sp.check(L.sp_opt_stepper_trial(h, 2.5, 7, None))  # accepted: 2.5 <= 3.0
    req, r = state(h)
    assert req.want == lib.OPT_WANT_DONE and r.converged == 1 and r.iterations == 0 and r.error == 2.5
    L.sp_opt_stepper_destroy(h)
    # ... and when every trial of that system is rejected, the solver's flag stands (:848)
    h = start(optimization_method="LM", max_iterations=1, lm_max_inner_iterations=2)
    sp.check(L.sp_opt_stepper_linearized(h, C.byref(bad)))
    sp.check(L.sp_opt_stepper_trial(h, 4.0, 7, None))
    sp.check(L.sp_opt_stepper_trial(h, 5.0, 7, None))
    req, r = state(h)
    assert req.want == lib.OPT_WANT_DONE and r.converged == 0 and r.trials == 2
    L.sp_opt_stepper_destroy(h)


def test_stepper_argument_errors(sp):
    lib, L = sp._lib, sp._lib.lib()
    op = sp.Registration(sp.RegistrationParams(optimization_method="LM", max_iterations=5)).opt_params()
    T0, h, req, r = colmajor(np.eye(4)), C.c_void_p(), lib.OptRequest(), lib.AlignResult()
    bad, sc = lib.SP_ERR_INVALID_ARGUMENT, floats(*([1.0] * (lib.OPT_MAX_LEVELS + 1)))
    assert L.sp_opt_stepper_create(None, T0.ctypes.data, sc, 1, C.byref(h)) == bad
    assert L.sp_opt_stepper_create(C.byref(op), None, sc, 1, C.byref(h)) == bad
    assert L.sp_opt_stepper_create(C.byref(op), T0.ctypes.data, None, 1, C.byref(h)) == bad
    assert L.sp_opt_stepper_create(C.byref(op), T0.ctypes.data, sc, 1, None) == bad
    assert L.sp_opt_stepper_create(C.byref(op), T0.ctypes.data, sc, lib.OPT_MAX_LEVELS + 1, C.byref(h)) == bad
    assert L.sp_opt_stepper_create(C.byref(op), T0.ctypes.data, sc, 0, C.byref(h)) == bad
    assert not h
    assert L.sp_opt_stepper_next(None, C.byref(req)) == bad and L.sp_opt_stepper_result(None, C.byref(r)) == bad
    assert L.sp_opt_stepper_linearized(None, C.byref(lib.Linearized())) == bad and L.sp_opt_stepper_trial(None, 1.0, 1, None) == bad
    sp.check(L.sp_opt_stepper_create(C.byref(op), T0.ctypes.data, sc, lib.OPT_MAX_LEVELS, C.byref(h)))
    assert L.sp_opt_stepper_next(h, None) == bad and L.sp_opt_stepper_result(h, None) == bad
    assert L.sp_opt_stepper_linearized(h, None) == bad
    # an answer of the wrong kind: a trial result while a linearisation is wanted, and the other way round; nothing changes
    sp.check(L.sp_opt_stepper_next(h, C.byref(req)))
    assert req.want == lib.OPT_WANT_LINEARIZE
    assert L.sp_opt_stepper_trial(h, 1.0, 10, None) == bad
    lin = lib.Linearized()
    for i in range(6):
        lin.H[i * 7] = 2.0
        lin.b[i] = 0.1
    lin.error, lin.inlier = 1.0, 10
    sp.check(L.sp_opt_stepper_linearized(h, C.byref(lin)))
    sp.check(L.sp_opt_stepper_next(h, C.byref(req)))
    assert req.want == lib.OPT_WANT_TRIAL
    assert L.sp_opt_stepper_linearized(h, C.byref(lin)) == bad
    sp.check(L.sp_opt_stepper_result(h, C.byref(r)))
    assert (r.linearizations, r.trials, r.pad[0]) == (1, 0, 0)
    L.sp_opt_stepper_destroy(h)
    L.sp_opt_stepper_destroy(None)
