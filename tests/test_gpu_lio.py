"""lio::LIORegistration on the device: the Python mirror here, the C++ facade through tests/cpp/test_lio_registration.cpp (built
with tests/cpp/Makefile's flags, as tests/test_gpu_lidar_odometry.py does). LIO adds no kernel: the device work is
Registration.compute_linearized_result / compute_error_frozen, the rest is the C library's stepper (sp_lio_stepper_*).

  1. align() is the stepper chain: GN / LM / DOGLEG x GICP / POINT_TO_PLANE x KDTree / GridKNN on the 600-of-900-point pair,
     against a loop in this file that drives the stepper by hand from a fresh Registration - bit for bit when two hand runs agree
     bit for bit, else within four times their largest difference (the rule of tests/test_gpu_lidar_odometry.py);
  2. one Gauss-Newton iteration with a valid prior against the float64 model (tests/f64_lio.py) fed with the device's sums:
     the bound and K of tests/test_lio_cpu.py;
  3. what the prior does, on the golden pair (box filter, voxel grid 0.25, k = 10 covariances) from the ground truth moved by
     (0.01, -0.005, 0.02 rad; 0.05, -0.04, 0.03 m): a loose prior (sigma = 1e3, directional weighting off) ends within TWICE the
     pose error of Registration.align with the same factor, optimiser and iteration budget (the chi-square weight and the
     15-dimensional damping change the path, not the minimum); a tight prior (1 / sigma^2 >= 100 |H_icp|_F, asserted on the
     device's linearisation) keeps |p - p_pred| and the rotation angle within 2 |b_icp| / h (delta = -(H + h I + lambda I)^-1 b
     with H positive semi-definite; 2 for the manifold's second order); the biases with and without update_bias; an invalid prior;
  4. the C++ program: reference-style code at the reference's six include paths, five known answers, (1) for LM / GICP / KDTree and
     (3) loose / tight.

Measured on an MI355X (every figure is printed by `pytest -s` before it is asserted): in all twelve cases of (1) two
hand runs are bit-identical and align() equals them bit for bit (2-3 iterations, 600 inliers), in the C++ facade too; (2) state
0.062 and posterior 0.005 of eps32 kappa scale (cond 103, K = 1); (3) on 6124 / 6096 points, translation / rotation error against
the ground truth, LIO with the loose prior | with the invalid prior | Registration.align: GN 0.00918 m / 0.00423 rad (4 iterations) |
the same | 0.00918 / 0.00423 (3); LM 0.00921 / 0.00428 (4) | the same | 0.00918 / 0.00423 (3); DOGLEG 0.00921 / 0.00428 (10) | the
same | 0.00921 / 0.00428 (9); tight prior, h = 101 |H_icp|_F = 3.35e9: |p - p_pred| 1.0e-5 m, angle 1.3e-4 rad, bound 3.8e-4, all
three optimisers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import f64_lio as M
from test_gpu_lidar_odometry import build

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CPP = os.path.join(ROOT, "tests", "cpp")
EPS = M.EPS32
TWIST = ((0.01, -0.005, 0.02), (0.05, -0.04, 0.03))


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    from sycl_points_amd import _lib

    _lib.build()
    import sycl_points_amd.api as api

    return api


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def with_features(sp, points, k):
    cloud = sp.PointCloudShared(points)
    sp.covariance.estimate(sp.KDTree.build(cloud.points).knn_search(cloud.points, k), cloud)
    sp.covariance.extract_normals(cloud)
    return cloud


@pytest.fixture(scope="module")
def small(sp):
    """the 600-of-900-point pair of gicp_pair(900, ...), covariances (k = 20) and normals from the library"""
    from sycl_points_amd.synthetic import gicp_pair

    src, tgt, T_gt = gicp_pair(900, 10.0 * (900 * 8.0 / 1e6) ** (1.0 / 3.0))
    source, target = with_features(sp, dev(src[:600]), 20), with_features(sp, dev(tgt), 20)
    return source, target, T_gt


@pytest.fixture(scope="module")
def golden(sp):
    from test_gpu_facade import read_ply_xyz

    def prep(path):
        pts = dev(read_ply_xyz(path))
        pts = sp.compact_by_flags(pts, sp.box_filter_flags(pts, 0.5, 50.0)).contiguous()
        cloud = sp.VoxelGrid(0.25).downsampling(sp.PointCloudShared(pts))
        return with_features(sp, cloud.points.contiguous(), 10)

    source, target = prep(os.path.join(GOLD, "source.ply")), prep(os.path.join(GOLD, "target.ply"))
    T_gt = np.loadtxt(os.path.join(GOLD, "T_target_source.txt"))
    return source, target, T_gt, sp.KDTree.build(target.points)


def moved(T_gt):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = M.rodrigues(np.array(TWIST[0])), TWIST[1]
    return np.asarray(T_gt, np.float64) @ T


def predicted(sp, T, seed=3):
    rs = np.random.RandomState(seed)
    T = np.asarray(T, np.float32)
    return sp.IMUState(T[:3, 3].copy(), T[:3, :3].copy(), np.array([0.3, -0.2, 0.1], np.float32),
                       np.array([0.02, -0.01, 0.03], np.float32), np.array([0.001, 0.002, -0.001], np.float32)), rs


def coupled_prior(rs, scale):
    Q, _ = np.linalg.qr(rs.normal(size=(15, 15)))
    P = (Q * rs.uniform(1.0, 4.0, 15)) @ Q.T * scale
    return ((P + P.T) / 2).astype(np.float32)


def hand_align(sp, factor, params, source, target, knn, pred, P, P_prev, update_bias):
    """LIORegistration.align written out: a fresh Registration serves the stepper."""
    lib, L = sp._lib, sp._lib.lib()
    reg = sp.Registration(factor)
    reg._validate(source, target)
    prm, facts = params.c_struct(), sp.lio_factor_facts(factor)
    h, req, res = C.c_void_p(), lib.LioRequest(), lib.LioResult()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cm = lambda A: np.ascontiguousarray(np.asarray(A, np.float32).T).reshape(-1)  # noqa: E731
    sp.check(L.sp_lio_stepper_create(C.byref(prm), C.byref(facts), vp(pred.pack()), vp(cm(P)), vp(cm(P_prev)), int(update_bias),
                                     C.byref(h)))
    try:
        while True:
            sp.check(L.sp_lio_stepper_next(h, C.byref(req)))
            if req.want == lib.OPT_WANT_DONE:
                break
            pose = np.array(req.T, np.float32).reshape(4, 4).T.copy()
            if req.want == lib.OPT_WANT_LINEARIZE:
                lin = reg.compute_linearized_result(source, target, knn, pose, req.robust_scale, req.rotation_robust_scale,
                                                    initial_pose=pred.pose())
                sp.check(L.sp_lio_stepper_linearized(h, C.byref(sp._lin6(lin))))
            else:
                e, n = reg.compute_error_frozen(source, target, pose, req.robust_scale, req.rotation_robust_scale)
                sp.check(L.sp_lio_stepper_trial(h, C.c_float(e), n))
        sp.check(L.sp_lio_stepper_result(h, C.byref(res)))
    finally:
        L.sp_lio_stepper_destroy(h)
    return (np.array(res.state, np.float32), np.array(res.posterior_covariance, np.float32).reshape(15, 15).T.copy(),
            int(res.iterations), int(res.inlier), np.float32(res.error))


def lio_params(sp, method, total, **kw):
    p = sp.LIORegistrationParams(total_iterations=total, optimization=sp.RegistrationParams(optimization_method=method))
    for k, v in kw.items():
        setattr(p.directional_icp_weighting if k == "enable" else p, k, v)
    return p


CHAIN = [(m, r, k) for m in ("GN", "LM", "DOGLEG") for r in ("GICP", "POINT_TO_PLANE") for k in ("KDTree", "GridKNN")]


@pytest.mark.parametrize("method,reg,knn", CHAIN, ids=["-".join(c) for c in CHAIN])
def test_align_is_the_stepper_chain(sp, small, method, reg, knn):
    source, target, T_gt = small
    tree = sp.KDTree.build(target.points) if knn == "KDTree" else sp.GridKNN.build(target.points)
    pred, rs = predicted(sp, moved(T_gt))
    P, P_prev = coupled_prior(rs, 1e-3), (np.eye(15) * 0.125).astype(np.float32)
    factor, params = sp.RegistrationParams(reg_type=reg), lio_params(sp, method, 6)
    a = hand_align(sp, factor, params, source, target, tree, pred, P, P_prev, True)
    b = hand_align(sp, factor, params, source, target, tree, pred, P, P_prev, True)
    r = sp.LIORegistration(factor, params).align(source, target, tree, pred, P, P_prev, True, 0.1, np.eye(4, dtype=np.float32))
    got = (r.state.pack(), r.posterior_covariance, r.registration_result.iterations, r.registration_result.inlier,
           np.float32(r.registration_result.error))
    spread = [float(np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)).max()) for x, y in zip(a, b)]
    diff = [float(np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)).max()) for x, y in zip(got, a)]
    print(f"\n[lio-chain] {method}-{reg}-{knn}: iterations {got[2]}, inlier {got[3]}, error {got[4]:.6g}; two hand runs differ by "
          f"{max(spread):.3g}, align() from the hand run by {max(diff):.3g}")
    assert 1 <= got[2] <= 6 and got[3] > 300 and r.registration_result.converged
    assert np.array_equal(r.registration_result.T, r.state.pose())
    for d, s in zip(diff, spread):
        assert d <= 4 * s  # (spread 0: bit for bit)


def test_one_iteration_against_float64_on_the_devices_sums(sp, small):
    source, target, T_gt = small
    tree = sp.KDTree.build(target.points)
    pred, rs = predicted(sp, moved(T_gt))
    P, P_prev = coupled_prior(rs, 1e-3), np.eye(15, dtype=np.float32)
    factor, params = sp.RegistrationParams(), lio_params(sp, "GN", 1)
    r = sp.LIORegistration(factor, params).align(source, target, tree, pred, P, P_prev, True, 0.1, np.eye(4, dtype=np.float32))
    lin = sp.Registration(factor).compute_linearized_result(source, target, tree, pred.pose(), initial_pose=pred.pose())
    assert (r.registration_result.iterations, r.registration_result.inlier) == (1, lin["inlier"])
    assert np.float32(r.registration_result.error) == np.float32(lin["error"])
    dirw = (True, 10.0, 10.0, 0.2, 0.2)

    def step(dt):
        x = M.St.unpack(pred.pack(), dt)
        H, b, _ = M.combined_system(lin, x, x, np.linalg.inv(P.astype(dt)), True, True, 3, dirw, 1e4, dt)
        d = -np.linalg.solve(H + dt(params.optimization.gn_lambda) * np.eye(15, dtype=dt), b)
        return M.retract(x, d).pack(), np.linalg.inv(H), d, H

    x64, P64, d64, H64 = step(np.float64)
    x32, P32, _, _ = step(np.float32)
    cond = lambda A: float(np.linalg.norm(A, np.inf) * np.linalg.norm(np.linalg.inv(A), np.inf))  # noqa: E731
    kd, kp = cond(H64 + params.optimization.gn_lambda * np.eye(15)), cond(H64)
    sx = kd * np.abs(d64).max() + max(1.0, np.abs(x64).max())
    spost = kp * np.abs(P64).max()
    K = max(1.0, np.abs(x32 - x64).max() / (EPS * sx), np.abs(P32 - P64).max() / (EPS * spost))
    ex, ep = np.abs(r.state.pack() - x64).max() / (EPS * sx), np.abs(r.posterior_covariance - P64).max() / (EPS * spost)
    print(f"\n[lio-f64-gpu] cond {kd:.1f} / {kp:.1f}; error / (eps32 kappa scale): state {ex:.3f}, posterior {ep:.3f}; numpy float32 K {K:.3f}")
    assert ex <= 4 * K and ep <= 4 * K


def pose_error(state, T_gt):
    dR = np.asarray(T_gt, np.float64)[:3, :3].T @ np.asarray(state.rotation, np.float64)
    return float(np.linalg.norm(state.position - np.asarray(T_gt)[:3, 3])), float(np.linalg.norm(M.log_so3(dR)))


def pose_error_T(T, T_gt):
    dR = np.asarray(T_gt, np.float64)[:3, :3].T @ np.asarray(T, np.float64)[:3, :3]
    return float(np.linalg.norm(np.asarray(T)[:3, 3] - np.asarray(T_gt)[:3, 3])), float(np.linalg.norm(M.log_so3(dR)))


@pytest.mark.parametrize("method", ["GN", "LM", "DOGLEG"])
def test_loose_prior_ends_where_registration_ends(sp, golden, method):
    """Measured on an MI355X (translation m / rotation rad, LIO then Registration.align): GN 0.00918 / 0.00423 then 0.00918 / 0.00423;
    LM 0.00921 / 0.00428 then 0.00918 / 0.00423; DOGLEG 0.00921 / 0.00428 then 0.00921 / 0.00428. The bound is twice the latter."""
    source, target, T_gt, tree = golden
    pred, rs = predicted(sp, moved(T_gt))
    factor = sp.RegistrationParams(optimization_method=method, max_iterations=10)
    ref = sp.Registration(factor).align(source, target, tree, pred.pose())
    P = (np.eye(15) * 1e6).astype(np.float32)
    r = sp.LIORegistration(factor, lio_params(sp, method, 10, enable=False)).align(source, target, tree, pred, P, P, True, 0.1,
                                                                                  np.eye(4, dtype=np.float32))
    (lt, lr), (rt, rr) = pose_error(r.state, T_gt), pose_error_T(ref.T, T_gt)
    print(f"\n[lio-prior] loose, {method}: LIO {lt:.5f} m / {lr:.5f} rad in {r.registration_result.iterations} iterations; "
          f"Registration.align {rt:.5f} m / {rr:.5f} rad in {ref.iterations}; {source.size()} / {target.size()} points")
    assert lt <= 2 * rt and lr <= 2 * rr
    # an invalid prior (zero covariance): velocity and biases untouched, the pose within the same bound
    r0 = sp.LIORegistration(factor, lio_params(sp, method, 10, enable=False)).align(
        source, target, tree, pred, np.zeros((15, 15), np.float32), P, True, 0.1, np.eye(4, dtype=np.float32))
    zt, zr = pose_error(r0.state, T_gt)
    print(f"[lio-prior] invalid prior, {method}: {zt:.5f} m / {zr:.5f} rad")
    assert np.array_equal(r0.state.pack()[12:], pred.pack()[12:])
    assert zt <= 2 * rt and zr <= 2 * rr


def test_tight_prior_keeps_the_prediction(sp, golden):
    source, target, T_gt, tree = golden
    pred, rs = predicted(sp, moved(T_gt))
    factor = sp.RegistrationParams()
    lin = sp.Registration(factor).compute_linearized_result(source, target, tree, pred.pose(), initial_pose=pred.pose())
    h = 101.0 * float(np.linalg.norm(lin["H"].astype(np.float64)))
    P = (np.eye(15) / h).astype(np.float32)
    assert 1.0 / float(P[0, 0]) >= 100.0 * np.linalg.norm(lin["H"].astype(np.float64))
    bound = 2.0 * float(np.linalg.norm(lin["b"].astype(np.float64))) / (1.0 / float(P[0, 0]))
    for method in ("GN", "LM", "DOGLEG"):
        r = sp.LIORegistration(factor, lio_params(sp, method, 10)).align(source, target, tree, pred, P, P, True, 0.1,
                                                                        np.eye(4, dtype=np.float32))
        dp = float(np.linalg.norm(r.state.position.astype(np.float64) - pred.position))
        da = float(np.linalg.norm(M.log_so3(pred.rotation.astype(np.float64).T @ r.state.rotation.astype(np.float64))))
        print(f"\n[lio-prior] tight, {method}: h {h:.4g}, |p - p_pred| {dp:.3g} m, angle {da:.3g} rad, bound {bound:.3g}")
        assert dp <= bound and da <= bound


def test_biases(sp, golden):
    source, target, T_gt, tree = golden
    pred, rs = predicted(sp, moved(T_gt))
    P = coupled_prior(rs, 1e-4)  # non-zero off-diagonal blocks: the pose correction reaches the biases
    lio = sp.LIORegistration(sp.RegistrationParams(), lio_params(sp, "GN", 5))
    frozen = lio.align(source, target, tree, pred, P, P, False, 0.1, np.eye(4, dtype=np.float32))
    free = lio.align(source, target, tree, pred, P, P, True, 0.1, np.eye(4, dtype=np.float32))
    assert np.array_equal(frozen.state.accel_bias, pred.accel_bias) and np.array_equal(frozen.state.gyro_bias, pred.gyro_bias)
    assert not np.array_equal(free.state.accel_bias, pred.accel_bias) and not np.array_equal(free.state.gyro_bias, pred.gyro_bias)
    assert not np.array_equal(frozen.state.position, pred.position)


def test_cpp_program(sp):
    exe = build(os.path.join(CPP, "test_lio_registration.cpp"), os.path.join(CPP, "test_lio_registration"))
    r = subprocess.run([exe, GOLD], capture_output=True, text=True, timeout=300)
    print(r.stdout[-12000:], r.stderr[-3000:])
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
    for name in ("known_answers_lio", "known_answers_imu", "align_is_the_stepper_chain", "loose_prior", "tight_prior"):
        assert f"[  OK  ] {name}" in r.stdout, name
