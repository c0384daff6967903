"""The sequential comparator of tests/test_gpu_voxel_align_batch.py: one alignment against a VoxelHashMap driven step by step
through the library's host stepper (sp_opt_stepper_*: the state machine the batch kernel runs on the device) with
Registration.linearize_voxel_map / error_voxel_map — two launches and a read-back per step, with annealing levels. No test.

trace() returns the final sp_align_result as a RegistrationResult, and per outer iteration
    trials, accepted, damping, error    (the stepper's own log)
    margin                              the smallest relative distance of any float comparison the optimiser branched on:
        LM       new_error against current_error:        |new - cur| / |new|
                 stagnation |new - last| against 1e-6:   ||new - last| - 1e-6| / |new|   (only where it is evaluated: new > cur)
        dog-leg  rho against eta1, and eta2 when taken:  |rho - eta| |predicted| / |new|, predicted = (cur - new) / rho
                 (each the relative change of the error sum `new` that would flip the comparison)
        all      the convergence test of the step the iteration ends on: |norm - criterion| / criterion for the rotation and the
                 translation part of sp_se3_log_host(T_lin^-1 T_step)
"""
import ctypes as C

import numpy as np

TINY = 1e-30


def _rel(a, b):
    return abs(a) / max(abs(b), TINY)


def _step_margin(L, T_from, T_to, op):
    """the convergence test on the step T_from -> T_to (column-major 16 floats each)"""
    A = np.asarray(T_from, np.float64).reshape(4, 4).T
    B = np.asarray(T_to, np.float64).reshape(4, 4).T
    D = np.ascontiguousarray((np.linalg.inv(A) @ B).T.astype(np.float32)).reshape(-1)
    tw = np.zeros(6, np.float32)
    L.sp_se3_log_host(D.ctypes.data_as(C.c_void_p), tw.ctypes.data_as(C.c_void_p))
    nr, nt = float(np.linalg.norm(tw[:3])), float(np.linalg.norm(tw[3:]))
    out = []
    if op.crit_rotation > 0:
        out.append(_rel(nr - op.crit_rotation, op.crit_rotation))
    if op.crit_translation > 0:
        out.append(_rel(nt - op.crit_translation, op.crit_translation))
    return min(out) if out else np.inf


def trace(sp, reg, source, voxel_map, T0, scales, neighbor_voxels=1):
    from sycl_points_amd import _lib

    L = _lib.lib()
    op, h, req, r = reg.opt_params(), C.c_void_p(), _lib.OptRequest(), _lib.AlignResult()
    method = op.method
    T = np.ascontiguousarray(np.asarray(T0, np.float32).T).reshape(-1).copy()
    sc = (C.c_float * len(scales))(*scales)
    if not voxel_map.registration_ready(reg.params.reg_type):
        voxel_map.prepare_registration(reg.params.reg_type)
    reg.prepare_voxel_source(source)
    sp.check(L.sp_opt_stepper_create(C.byref(op), T.ctypes.data_as(C.c_void_p), sc, len(scales), C.byref(h)))
    margins, cur_margin = [], np.inf
    cur_error, last_error = 0.0, np.finfo(np.float32).max
    n_logged = 0

    def close_iterations():
        nonlocal n_logged, cur_margin
        sp.check(L.sp_opt_stepper_result(h, C.byref(r)))
        while n_logged < r.log_entries:
            margins.append(cur_margin)
            n_logged += 1
        cur_margin = np.inf

    try:
        while True:
            sp.check(L.sp_opt_stepper_next(h, C.byref(req)))
            if req.want == _lib.OPT_WANT_DONE:
                break
            Tq = np.array(req.T, np.float32)
            pose = Tq.reshape(4, 4).T
            if req.want == _lib.OPT_WANT_LINEARIZE:
                lr = reg.linearize_voxel_map(source, voxel_map, pose, req.robust_scale, neighbor_voxels, prepare_source=False)["lin"]
                cur_error, last_error = float(lr.error), np.finfo(np.float32).max
                sp.check(L.sp_opt_stepper_linearized(h, C.byref(lr)))
                if method == 0:  # Gauss-Newton: the step is taken at once, the iteration ends on its convergence test
                    sp.check(L.sp_opt_stepper_result(h, C.byref(r)))
                    cur_margin = min(cur_margin, _step_margin(L, Tq, np.array(r.T, np.float32), op))
                    close_iterations()
                else:
                    close_iterations()  # (an iteration that ended without a trial: LM with no inner iterations, a dog-leg step that predicts no gain)
            else:
                new, inl = reg.error_voxel_map(source, voxel_map, pose, req.robust_scale)
                new = float(np.float32(new))
                rho = C.c_float(0.0)
                T_lin = np.array(req.T_lin, np.float32)
                step = _step_margin(L, T_lin, Tq, op)
                if method == 1:
                    cur_margin = min(cur_margin, _rel(new - cur_error, new))
                    if new > cur_error:
                        cur_margin = min(cur_margin, _rel(abs(new - last_error) - 1e-6, new))
                    last_error = new
                sp.check(L.sp_opt_stepper_trial(h, C.c_float(new), inl, C.byref(rho)))
                if method == 2 and rho.value != 0.0:
                    pred = (cur_error - new) / rho.value
                    cur_margin = min(cur_margin, _rel((rho.value - op.dl_eta1) * pred, new))
                    if rho.value >= op.dl_eta1:
                        cur_margin = min(cur_margin, _rel((rho.value - op.dl_eta2) * pred, new))
                before = n_logged
                sp.check(L.sp_opt_stepper_result(h, C.byref(r)))
                if r.log_entries > before:  # this trial ended the iteration: its step's convergence test was (or may have been) used
                    cur_margin = min(cur_margin, step)
                    close_iterations()
        sp.check(L.sp_opt_stepper_result(h, C.byref(r)))
    finally:
        L.sp_opt_stepper_destroy(h)
    res = reg._result_from_align_result(r)
    assert len(res.log) == len(margins) or r.log_entries == _lib.OPT_LOG_ENTRIES
    steps = [dict(trials=e["trials"], accepted=e["accepted"], damping=e["damping"], error=e["error"], margin=float(m))
             for e, m in zip(res.log, margins)]
    return res, steps
