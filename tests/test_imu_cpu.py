"""IMU preintegration and IMU deskew without a device: the C ABI's exports and argument checks (sp_deskew_imu returns
SP_ERR_INVALID_ARGUMENT before any HIP call), the reference's known answers (cpp/tests/test_imu_preintegration.cpp, every TEST with
its own tolerance; the status and coverage cases of cpp/tests/test_imu_deskew.cpp through the C call and through api), the host
integrator against a float64 evaluation of the same recurrences, sp_imu_deskew_intervals_host bit for bit against the per-point
slerp of the CPU restatement of the kernel (tests/cpp/imu_deskew_restate.cpp; deskew/imu_deskew.hpp:330-411), and the exact
properties of that restatement the GPU suite (tests/test_gpu_imu_deskew.py) then holds the device to bit for bit.

The integrator's yardstick: np_integrator(np.float64) evaluates the recurrences of imu_preintegration.hpp:356-519 and the
trajectory of imu_deskew.hpp:158-285 in float64 from the same float32 samples; np_integrator(np.float32) is a plain float32
transcription in the reference's order. E_ref is the transcription's largest absolute error against the yardstick, E_lib the
library's, per quantity, and the library passes when E_lib <= 4 * E_ref: the 4 covers the reassociation inside three-factor
products, which Eigen leaves unpinned, not a different formula. Both are printed before the assertion (run with -s).

(Bit-identity at t <= 0 is stated for coordinates that are not -0.0: the fma chain of multiply<3,3> starts from +0, so a -0.0
coordinate comes out +0.0, in the reference as here.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
GRAVITY = (0.0, 0.0, -9.80665)


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def api(L):
    import sycl_points_amd.api as api

    return api


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libimu_deskew_restate.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "imu_deskew_restate.cpp"), "-o", so])
    R = C.CDLL(so)
    for name in ("imu_deskew_restate", "imu_deskew_f64"):
        fn = getattr(R, name)
        fn.restype = None
        fn.argtypes = [_vp, _vp, _vp, _vp, C.c_uint64, _vp, C.c_uint64, _vp, _vp, _vp]
    R.imu_intervals_restate.restype = None
    R.imu_intervals_restate.argtypes = [_vp, C.c_uint64, _vp, _vp]
    return R


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return build_restatement(tmp_path_factory.mktemp("imu_deskew"))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def restate(R, pts, covs, nrm, t_ms, traj, f64=False, in_place=False):
    """(points, covs, normals) of the restatement (float32) or of the float64 evaluation; missing attributes stay None"""
    dt = np.float64 if f64 else np.float32
    assert not (f64 and in_place)
    pts, t_ms = np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(t_ms, np.float32)
    covs = None if covs is None else np.ascontiguousarray(covs, np.float32)
    nrm = None if nrm is None else np.ascontiguousarray(nrm, np.float32)
    if in_place:
        po, co, no = pts.copy(), None if covs is None else covs.copy(), None if nrm is None else nrm.copy()
        pts, covs, nrm = po, co, no
    else:
        po = np.empty(pts.shape, dt)
        co = None if covs is None else np.empty(covs.shape, dt)
        no = None if nrm is None else np.empty(nrm.shape, dt)
    tr = np.ascontiguousarray(traj, np.float32)
    (R.imu_deskew_f64 if f64 else R.imu_deskew_restate)(_ptr(pts), _ptr(covs), _ptr(nrm), _ptr(t_ms), len(pts), _ptr(tr), len(tr),
                                                        _ptr(po), _ptr(co), _ptr(no))
    return po, co, no


def random_cloud(n, seed=1234):
    """U(-50, 50) points (w = 1), unit normals, random symmetric positive covariances in the top-left 3x3 of a 4x4 whose fourth
    row and column hold a marker (so that a copied row can be told from a recomputed one)."""
    rs = np.random.RandomState(seed)
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = rs.uniform(-50, 50, (n, 3))
    nr = rs.normal(size=(n, 3))
    nrm = np.zeros((n, 4), np.float32)
    nrm[:, :3] = nr / np.linalg.norm(nr, axis=1, keepdims=True)
    A = rs.normal(size=(n, 3, 3)).astype(np.float32) * np.float32(0.1)
    covs = np.zeros((n, 4, 4), np.float32)
    covs[:, :3, :3] = A @ A.transpose(0, 2, 1) + np.float32(1e-3) * np.eye(3, dtype=np.float32)
    covs[:, :3, :3] = 0.5 * (covs[:, :3, :3] + covs[:, :3, :3].transpose(0, 2, 1))
    covs[:, 3, 3] = 7.0  # marker: only a copied row keeps it
    return pts, covs.reshape(n, 16), nrm


def synthetic_trajectory(n_traj, gyro_rate, accel, duration=0.1, seed=3, equal_pair=True):
    """n_traj poses of a smooth motion over [0, duration]: the identity at stamp 0, then rotation about a fixed axis at gyro_rate
    rad/s with a small wobble, translation 0.5 * accel * t^2 along a fixed direction. With equal_pair and n_traj >= 6 two
    neighbouring poses share a stamp (alpha = 0 there). float32 (n_traj, 8): q xyzw, t xyz, stamp."""
    rs = np.random.RandomState(seed)
    ax, d = rs.normal(size=3), rs.normal(size=3)
    ax, d = ax / np.linalg.norm(ax), d / np.linalg.norm(d)
    t = np.linspace(0.0, duration, n_traj)
    if equal_pair and n_traj >= 6:
        t[n_traj // 2] = t[n_traj // 2 - 1]
    traj = np.zeros((n_traj, 8), np.float32)
    for i, ti in enumerate(t):
        a = ax + 0.05 * np.array([np.sin(40 * ti), np.cos(31 * ti) - 1.0, np.sin(23 * ti)])
        ang = gyro_rate * ti
        a = a / np.linalg.norm(a)
        traj[i, :3] = np.sin(0.5 * ang) * a
        traj[i, 3] = np.cos(0.5 * ang)
        traj[i, 4:7] = 0.5 * accel * ti * ti * d
        traj[i, 7] = ti
    traj[0] = [0, 0, 0, 1, 0, 0, 0, 0]
    return traj


# ------------------------------------------------------------------------------------------------ C ABI
NEW_SYMBOLS = ("sp_imu_preint_create", "sp_imu_preint_destroy", "sp_imu_preint_reset", "sp_imu_preint_integrate",
               "sp_imu_preint_num_measurements", "sp_imu_preint_get", "sp_imu_preint_predict_relative",
               "sp_imu_preint_predict_transform", "sp_imu_deskew_trajectory_host", "sp_imu_deskew_intervals_host", "sp_deskew_imu")


def test_symbols_exported_and_listed(L):
    from sycl_points_amd import _lib

    with open(os.path.join(ROOT, "include", "sycl_points_amd.h")) as f:
        hdr = f.read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
        assert name + "(" in hdr
    assert L.sp_abi_version() == 7
    assert C.sizeof(_lib.ImuParams) == 32 and C.sizeof(_lib.ImuState) == 1152


def test_invalid_arguments_need_no_device(L):
    from sycl_points_amd import _lib

    a = np.zeros((8, 16), np.float32)
    P = _ptr(a)
    ok = dict(points=P, covs=None, normals=None, ts=P, n=8, rows=P, m=1, po=P, co=None, no=None)
    cases = [dict(points=None), dict(ts=None), dict(po=None), dict(rows=None),
             dict(covs=P), dict(co=P), dict(normals=P), dict(no=P),             # an attribute without its other half
             dict(m=0), dict(m=1 << 31), dict(n=1 << 32), dict(n=(1 << 32) + 5)]
    for c in cases:
        k = {**ok, **c}
        rc = L.sp_deskew_imu(k["points"], k["covs"], k["normals"], k["ts"], k["n"], k["rows"], k["m"], k["po"], k["co"], k["no"], None)
        assert rc == _lib.SP_ERR_INVALID_ARGUMENT, c
        assert b"sp_deskew_imu" in L.sp_last_error()
    # n == 0: SP_OK, nothing enqueued (no device is needed for it)
    assert L.sp_deskew_imu(P, None, None, P, 0, P, 1, P, None, None, None) == 0
    assert L.sp_imu_deskew_intervals_host(P, 1, P) == _lib.SP_ERR_INVALID_ARGUMENT
    assert L.sp_imu_deskew_intervals_host(None, 2, P) == _lib.SP_ERR_INVALID_ARGUMENT
    assert L.sp_imu_preint_get(None, None, None) == _lib.SP_ERR_INVALID_ARGUMENT


def test_resource_report_has_no_scratch(L):
    path = os.path.join(ROOT, "sycl_points_amd", "lib", "imu_deskew.resources.txt")
    with open(path) as f:
        rows = [r for r in f.read().splitlines() if "imu_deskew_kernel" in r]
    assert len(rows) == 4, rows  # points | + covs | + normals | + both
    for r in rows:
        assert re.search(r"VGPRs Spill: 0\b", r) and re.search(r"ScratchSize \[bytes/lane\]: 0\b", r), r


# ------------------------------------------------------------------------------------------------ known answers: preintegration
kEps, kEpsTight = 1e-4, 1e-5


def make_constant_imu(t0, T, n_steps, gyro, accel):
    dt = T / n_steps
    return [(t0 + i * dt, np.array(gyro, np.float32), np.array(accel, np.float32)) for i in range(n_steps + 1)]


def feed(integ, meas):
    for t, g, a in meas:
        integ.integrate(t, g, a)
    return integ


def is_approx(a, b, prec):  # Eigen's isApprox: |a - b| <= prec * min(|a|, |b|) in the Frobenius norm
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) <= prec * min(np.linalg.norm(a), np.linalg.norm(b))


def is_zero(a, prec):  # Eigen's isZero
    return bool((np.abs(a) <= prec).all())


def rot_z(angle):
    c, s = np.cos(np.float32(angle)), np.sin(np.float32(angle))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)


NOISY = dict(gyro_noise_density=1e-3, accel_noise_density=1e-2, gyro_bias_rw_density=1e-5, accel_bias_rw_density=1e-4)


def test_reference_preintegration_cases(api):
    """cpp/tests/test_imu_preintegration.cpp, TEST by TEST (the numbers are the reference's)"""
    I3 = np.eye(3, dtype=np.float32)
    new = lambda **kw: api.IMUPreintegration(api.IMUPreintegrationParams(**kw))  # noqa: E731
    # 1 InitialStateIsIdentity
    integ = new()
    assert not integ.has_measurements() and integ.get_dt_total() == 0.0
    r = integ.get_raw()
    assert is_approx(r.Delta_R, I3, kEpsTight) and is_zero(r.Delta_v, kEpsTight) and is_zero(r.Delta_p, kEpsTight)
    # 2 ResetClearsState
    feed(integ, make_constant_imu(0.0, 1.0, 100, (0.1, 0, 0), (0, 0, 9.81)))
    assert integ.has_measurements()
    integ.reset()
    assert not integ.has_measurements() and integ.get_dt_total() == 0.0
    r = integ.get_raw()
    assert is_approx(r.Delta_R, I3, kEpsTight) and is_zero(r.Delta_v, kEpsTight) and is_zero(r.Delta_p, kEpsTight)
    # 3 SingleMeasurementNoIntegration
    integ = new()
    integ.integrate(1.0, (0.1, 0.2, 0.3), (0, 0, 9.81))
    assert integ.has_measurements() and integ.get_dt_total() == 0.0 and is_approx(integ.get_raw().Delta_R, I3, kEpsTight)
    # 4 ZeroMotionIdentityResult
    r = feed(new(), make_constant_imu(0.0, 1.0, 200, (0, 0, 0), (0, 0, 0))).get_raw()
    assert is_approx(r.Delta_R, I3, kEps) and is_zero(r.Delta_v, kEps) and is_zero(r.Delta_p, kEps) and abs(r.dt_total - 1.0) <= 1e-9
    # 5 ConstantRotationZ
    omega_z = np.float32(np.pi) / np.float32(4.0)
    r = feed(new(), make_constant_imu(0.0, 2.0, 400, (0, 0, omega_z), (0, 0, 0))).get_raw()
    assert is_approx(r.Delta_R, rot_z(omega_z * np.float32(2.0)), kEps)
    # 6 ConstantAccelerationX
    r = feed(new(), make_constant_imu(0.0, 1.5, 300, (0, 0, 0), (2.0, 0, 0))).get_raw()
    assert abs(r.Delta_p[0] - 0.5 * 2.0 * 1.5 * 1.5) <= kEps and abs(r.Delta_p[1]) <= kEps and abs(r.Delta_p[2]) <= kEps
    assert abs(r.Delta_v[0] - 2.0 * 1.5) <= kEps
    # 7 BatchAndIncrementalAreEqual
    meas = make_constant_imu(0.0, 1.0, 100, (0.05, -0.03, 0.08), (0.3, -0.1, 9.5))
    ri = feed(new(), meas).get_raw()
    batch = new()
    batch.integrate_batch(*zip(*meas))
    rb = batch.get_raw()
    assert is_approx(ri.Delta_R, rb.Delta_R, kEpsTight) and is_approx(ri.Delta_v, rb.Delta_v, kEpsTight)
    assert is_approx(ri.Delta_p, rb.Delta_p, kEpsTight) and ri.dt_total == rb.dt_total
    # 8 BiasCorrection_SmallChange
    gyro, accel = (0.1, -0.05, 0.08), (0.2, 0.1, 9.7)
    b0 = np.array([0.005, -0.003, 0.002, 0.01, 0.005, -0.008], np.float32)
    b1 = b0 + np.array([0.001, -0.001, 0.001, 0.002, 0.001, -0.001], np.float32)
    ref, foc = new(), new()
    ref.reset(b1)
    foc.reset(b0)
    r_ref = feed(ref, make_constant_imu(0.0, 0.5, 100, gyro, accel)).get_raw()
    r_cor = feed(foc, make_constant_imu(0.0, 0.5, 100, gyro, accel)).get_corrected(b1)
    assert is_approx(r_cor.Delta_R, r_ref.Delta_R, 5e-3) and is_approx(r_cor.Delta_v, r_ref.Delta_v, 5e-3)
    assert is_approx(r_cor.Delta_p, r_ref.Delta_p, 5e-3)
    # 9 PredictRelativeTransformZeroMotion
    integ = feed(new(), make_constant_imu(0.0, 0.5, 50, (0, 0, 0), tuple(-g for g in GRAVITY)))
    assert is_approx(integ.predict_relative_transform(I3, (0, 0, 0)), np.eye(4), kEps)
    # 10 PredictTransform_FreeFall
    integ = feed(new(gravity=(0, 0, -9.81)), make_constant_imu(0.0, 1.0, 200, (0, 0, 0), (0, 0, 0)))
    Tj = integ.predict_transform(np.eye(4), (0, 0, 0))
    assert abs(Tj[0, 3]) <= kEps and abs(Tj[1, 3]) <= kEps and abs(Tj[2, 3] - np.float32(0.5) * np.float32(-9.81)) <= kEps
    assert is_approx(Tj[:3, :3], I3, kEps)
    # 11 PredictTransform_InitialVelocity
    integ = feed(new(gravity=(0, 0, -9.81)), make_constant_imu(0.0, 2.0, 400, (0, 0, 0), (0, 0, 0)))
    Ti = np.eye(4, dtype=np.float32)
    Ti[:3, 3] = [1, 2, 3]
    Tj = integ.predict_transform(Ti, (1.0, -0.5, 0.0))
    exp = np.array([1 + 2.0, 2 - 0.5 * 2.0, 3 + np.float32(0.5) * np.float32(-9.81) * np.float32(4.0)], np.float32)
    assert np.abs(Tj[:3, 3] - exp).max() <= kEps
    # 12 DeltaRRemainsValidRotation
    Rm = feed(new(), make_constant_imu(0.0, 5.0, 500, (0.3, -0.2, 0.5), (0.1, 0.2, 9.5))).get_raw().Delta_R
    assert abs(np.linalg.det(Rm.astype(np.float64)) - 1.0) <= 1e-4 and is_approx(Rm.T @ Rm, I3, 1e-4)
    # 13 MidpointBetterThanEulerForRotation
    Rm = feed(new(), make_constant_imu(0.0, 2.0, 20, (0, 0, 1.5), (0, 0, 0))).get_raw().Delta_R
    assert np.linalg.norm(Rm - rot_z(np.float32(1.5) * np.float32(2.0))) < 0.01
    # 14 CovarianceZeroWithNoNoise
    assert is_zero(feed(new(), make_constant_imu(0.0, 1.0, 100, (0.1, 0, 0), (0, 0, 9.81))).get_raw().covariance, kEpsTight)
    # 15 CovarianceGrowsWithNoise
    cov = feed(new(**NOISY), make_constant_imu(0.0, 1.0, 100, (0, 0, 0), (0, 0, 0))).get_raw().covariance
    assert cov[3, 3] > 0 and cov[6, 6] > 0 and cov[0, 0] > 0 and cov[9, 9] > 0 and cov[12, 12] > 0
    # 16 CovarianceIsSymmetric, 17 CovarianceIsPositiveSemiDefinite
    cov = feed(new(**NOISY), make_constant_imu(0.0, 1.0, 100, (0.1, -0.05, 0.08), (0.2, 0.1, 9.7))).get_raw().covariance
    assert is_approx(cov, cov.T, 1e-5)
    assert np.linalg.eigvalsh(cov.astype(np.float64)).min() >= -1e-6
    # 18 InitialCovariancePropagatedForward
    P0 = np.diag(np.repeat([1e-4, 1e-6, 1e-4, 1e-8, 1e-8], 3)).astype(np.float32)
    integ = new(**NOISY)
    integ.reset(None, P0)
    cov = feed(integ, make_constant_imu(0.0, 1.0, 100, (0, 0, 0), (0, 0, 0))).get_raw().covariance
    assert cov[3, 3] >= P0[3, 3] and cov[6, 6] >= P0[6, 6] and cov[0, 0] > P0[0, 0]
    # 19 ZeroNoiseNoStepPreservesCovariance
    P0 = (np.eye(15) * 1e-4).astype(np.float32)
    integ = new()
    integ.reset(None, P0)
    integ.integrate(0.0, (0, 0, 0), (0, 0, 0))
    assert is_approx(integ.get_raw().covariance, P0, kEpsTight)
    # 20 ZeroNoisePropagatesInitialCovariance
    P0 = np.zeros((15, 15), np.float32)
    P0[6:9, 6:9] = 1e-4 * np.eye(3)
    integ = new()
    integ.reset(None, P0)
    cov = feed(integ, make_constant_imu(0.0, 1.0, 100, (0, 0, 0), (0, 0, 0))).get_raw().covariance
    assert abs(cov[6, 6] - P0[6, 6]) <= 1e-6 and cov[0, 0] > 0 and cov[1, 1] > 0 and cov[2, 2] > 0
    # 21 GetCorrectedSameBiasEqualsRaw
    bias = np.array([0.01, -0.02, 0.005, 0.05, 0.02, -0.01], np.float32)
    integ = new()
    integ.reset(bias)
    feed(integ, make_constant_imu(0.0, 1.0, 100, (0.1, 0, 0), (0, 0, 9.81)))
    raw, cor = integ.get_raw(), integ.get_corrected(bias)
    assert is_approx(cor.Delta_R, raw.Delta_R, kEpsTight) and is_approx(cor.Delta_v, raw.Delta_v, kEpsTight)
    assert is_approx(cor.Delta_p, raw.Delta_p, kEpsTight)
    # 22 MidpointGyroBiasJacobiansMatchFiniteDifference
    meas, eps = make_constant_imu(0.0, 0.2, 1, (0.2, -0.1, 1.0), (4.0, 1.0, 8.0)), np.float32(1e-2)
    nominal = feed(new(), meas).get_raw()
    plus, minus = new(), new()
    plus.reset([0, 0, eps, 0, 0, 0])
    minus.reset([0, 0, -eps, 0, 0, 0])
    rp, rm = feed(plus, meas).get_raw(), feed(minus, meas).get_raw()
    assert is_approx(nominal.J_v_bg[:, 2], (rp.Delta_v - rm.Delta_v) / (np.float32(2.0) * eps), 5e-4)
    assert is_approx(nominal.J_p_bg[:, 2], (rp.Delta_p - rm.Delta_p) / (np.float32(2.0) * eps), 5e-4)
    # 23 CovarianceUsesWorldFrameAtReset
    dt, Rwb, accel = np.float32(0.1), rot_z(np.float32(np.pi) / np.float32(2.0)), np.array([1.0, 2.0, 9.0], np.float32)
    P0 = np.zeros((15, 15), np.float32)
    P_rot = np.diag([1e-4, 2e-4, 3e-4]).astype(np.float32)
    P0[3:6, 3:6] = P_rot
    integ = new()
    integ.reset(None, P0, Rwb)
    feed(integ, make_constant_imu(0.0, 0.1, 1, (0, 0, 0), accel))
    S = np.array([[0, -accel[2], accel[1]], [accel[2], 0, -accel[0]], [-accel[1], accel[0], 0]], np.float32)
    A = -Rwb @ S * dt
    assert is_approx(integ.get_raw().covariance[6:9, 6:9], A @ P_rot @ A.T, 1e-6)
    # 24 GyroNoiseCouplesIntoPositionAndVelocity
    cov = feed(new(gyro_noise_density=1e-2), make_constant_imu(0.0, 0.1, 1, (0, 0, 1.0), (4.0, 1.0, 8.0))).get_raw().covariance
    assert np.trace(cov[0:3, 0:3]) > 0 and np.trace(cov[6:9, 6:9]) > 0 and np.linalg.norm(cov[6:9, 3:6]) > 0
    # 25 MeasurementWindowInterpolatesBoundaries
    meas = [(float(i), np.full(3, float(i), np.float32), np.full(3, 10.0 * i, np.float32)) for i in range(3)]
    w = api.build_measurement_window(meas, 0.25, 1.75)
    assert len(w) == 3 and w[0][0] == 0.25 and w[1][0] == 1.0 and w[2][0] == 1.75
    assert is_approx(w[0][1], np.full(3, 0.25), 1e-5) and is_approx(w[2][2], np.full(3, 17.5), 1e-5)


# ------------------------------------------------------------------------------------------------ known answers: deskew status
def make_imu_buffer(t0, T, n_steps, gyro, accel):
    dt = T / n_steps
    stamps = np.array([t0 + i * dt for i in range(n_steps + 1)], np.float64)
    return stamps, np.tile(np.array(gyro, np.float32), (n_steps + 1, 1)), np.tile(np.array(accel, np.float32), (n_steps + 1, 1))


def c_trajectory(L, stamps, gyro, accel, scan_start, duration, gyro_only=False, gravity=GRAVITY, bias=None, T_il=None, Rwb=None,
                 v=None, noise=None, capacity=None):
    """sp_imu_deskew_trajectory_host: (rc, status, trajectory)"""
    from sycl_points_amd import _lib

    n = len(stamps)
    ga = np.ascontiguousarray(np.concatenate([np.asarray(gyro, np.float32).reshape(n, 3), np.asarray(accel, np.float32).reshape(n, 3)],
                                             axis=1)) if n else np.zeros((0, 6), np.float32)
    stamps = np.ascontiguousarray(stamps, np.float64)
    cap = n + 1 if capacity is None else capacity
    traj = np.zeros((max(cap, 1), 8), np.float32)
    T = np.ascontiguousarray((np.eye(4) if T_il is None else np.asarray(T_il)).T, np.float32)
    Rm = np.ascontiguousarray((np.eye(3) if Rwb is None else np.asarray(Rwb)).T, np.float32)
    vv = np.zeros(3, np.float32) if v is None else np.ascontiguousarray(v, np.float32)
    b = np.zeros(6, np.float32) if bias is None else np.ascontiguousarray(bias, np.float32)
    prm = _lib.ImuParams((C.c_float * 3)(*gravity), 1.0, *(noise or (0.0, 0.0, 0.0, 0.0)))
    m, status = C.c_size_t(99), C.c_int(99)
    rc = L.sp_imu_deskew_trajectory_host(_ptr(stamps), _ptr(ga), n, scan_start, duration, _ptr(T), _ptr(b), C.byref(prm), _ptr(Rm),
                                         _ptr(vv), int(gyro_only), _ptr(traj), cap, C.byref(m), C.byref(status))
    return rc, status.value, traj[:m.value].copy()


def test_reference_deskew_status_cases(L, api):
    """cpp/tests/test_imu_deskew.cpp:259-352 through the C call and through api (a cloud on the host is enough: every case
    returns before the device is touched)"""
    from sycl_points_amd import _lib

    S = api.IMUDeskewStatus
    one = np.array([[1.0, 0.0, 0.0, 1.0]], np.float32)

    def cloud(start_ms, end_ms, stamps=True, empty=False):
        pc = api.PointCloudShared.from_numpy(one[:0] if empty else one, device="cpu",
                                             timestamp_offsets=np.zeros(0 if empty else 1, np.float32) if stamps else None)
        pc.start_time_ms, pc.end_time_ms = start_ms, end_ms
        return pc

    full = make_imu_buffer(0.98, 0.14, 20, (0, 0, 0), (0, 0, 9.81))
    # InsufficientIMUDataReturnsFalse: an empty buffer
    empty = (np.zeros(0), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    rc, st, tr = c_trajectory(L, *empty, 1.0, 0.1)
    assert (rc, st, len(tr)) == (0, _lib.IMU_DESKEW_STATUS.index("insufficient_imu_coverage"), 0)
    assert api.deskew_point_cloud_imu(cloud(1000.0, 1100.0), *empty, 1.0, np.eye(4)) == (None, S.insufficient_imu_coverage)
    # NoTimestampsReturnsFalse
    assert api.deskew_point_cloud_imu(cloud(1000.0, 1100.0, stamps=False), *full, 1.0, np.eye(4)) == (None, S.no_timestamps)
    # ZeroScanDurationReturnsFalse
    rc, st, tr = c_trajectory(L, *full, 1.0, 0.0)
    assert (rc, st, len(tr)) == (0, _lib.IMU_DESKEW_STATUS.index("invalid_scan_duration"), 0)
    assert c_trajectory(L, *full, 1.0, -0.5)[1] == S.invalid_scan_duration
    assert api.deskew_point_cloud_imu(cloud(1000.0, 1000.0), *full, 1.0, np.eye(4)) == (None, S.invalid_scan_duration)
    # PartialIMUCoverageReturnsFalse: [0.98, 1.04] against scan end 1.1
    part = make_imu_buffer(0.98, 0.06, 10, (0, 0, 0), (0, 0, 9.81))
    rc, st, tr = c_trajectory(L, *part, 1.0, 0.1)
    assert (rc, st, len(tr)) == (0, S.insufficient_imu_coverage, 0)
    assert api.deskew_point_cloud_imu(cloud(1000.0, 1100.0), *part, 1.0, np.eye(4)) == (None, S.insufficient_imu_coverage)
    # an empty cloud (imu_deskew.hpp:141-145)
    assert api.deskew_point_cloud_imu(cloud(1000.0, 1100.0, empty=True), *full, 1.0, np.eye(4)) == (None, S.empty_cloud)
    # the full buffer succeeds: the identity first, stamps from scan start on, the last one within 50 ms of the scan's end
    rc, st, tr = c_trajectory(L, *full, 1.0, 0.1)
    assert (rc, st) == (0, S.success) and len(tr) >= 2
    assert np.array_equal(tr[0], np.array([0, 0, 0, 1, 0, 0, 0, 0], np.float32))
    assert (tr[1:, 7] >= 0).all() and (np.diff(tr[:, 7]) >= 0).all() and tr[-1, 7] >= 0.1 - 0.05
    t2, st2 = api.imu_deskew_trajectory(*full, 1.0, 0.1, np.eye(4))
    assert st2 == S.success and np.array_equal(t2.view(np.uint32), tr.view(np.uint32))
    # a trajectory that does not fit is an error, not a truncation
    assert c_trajectory(L, *full, 1.0, 0.1, capacity=3)[0] == _lib.SP_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------ the integrator against float64
def np_integrator(D):
    """The recurrences of imu_preintegration.hpp:180-529 and the trajectory of imu_deskew.hpp:158-285 with every operation in
    dtype D, in the reference's order; matrix products are numpy's. Returns a namespace of functions."""
    f = D
    I3 = np.eye(3, dtype=D)

    def skew(x):
        return np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]], D)

    def so3_exp(w):
        th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
        if th2 < f(1e-6):
            t4 = th2 * th2
            imag = f(0.5) - f(1.0) / f(48.0) * th2 + f(1.0) / f(3840.0) * t4
            real = f(1.0) - f(1.0) / f(8.0) * th2 + f(1.0) / f(384.0) * t4
        else:
            th = np.sqrt(th2)
            imag, real = np.sin(f(0.5) * th) / th, np.cos(f(0.5) * th)
        return np.array([imag * w[0], imag * w[1], imag * w[2], real], D)

    def q2r(q):
        x, y, z, w = q
        two, one = f(2.0), f(1.0)
        return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                         [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                         [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], D)

    def r2q(R):
        tr = R[0, 0] + R[1, 1] + R[2, 2]
        one, two, q4 = f(1.0), f(2.0), f(0.25)
        if tr > 0:
            S = np.sqrt(tr + one) * two
            return np.array([(R[2, 1] - R[1, 2]) / S, (R[0, 2] - R[2, 0]) / S, (R[1, 0] - R[0, 1]) / S, q4 * S], D)
        if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
            S = np.sqrt(one + R[0, 0] - R[1, 1] - R[2, 2]) * two
            return np.array([q4 * S, (R[0, 1] + R[1, 0]) / S, (R[0, 2] + R[2, 0]) / S, (R[2, 1] - R[1, 2]) / S], D)
        if R[1, 1] > R[2, 2]:
            S = np.sqrt(one + R[1, 1] - R[0, 0] - R[2, 2]) * two
            return np.array([(R[0, 1] + R[1, 0]) / S, q4 * S, (R[1, 2] + R[2, 1]) / S, (R[0, 2] - R[2, 0]) / S], D)
        S = np.sqrt(one + R[2, 2] - R[0, 0] - R[1, 1]) * two
        return np.array([(R[0, 2] + R[2, 0]) / S, (R[1, 2] + R[2, 1]) / S, q4 * S, (R[1, 0] - R[0, 1]) / S], D)

    def jr(phi):
        th = np.sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2])
        S = skew(phi)
        S2 = S @ S
        if th < f(1e-4):
            return I3 - f(0.5) * S + (f(1.0) / f(6.0)) * S2
        return I3 - (f(1.0) - np.cos(th)) / (th * th) * S + (th - np.sin(th)) / (th * th * th) * S2

    class Integ:
        def __init__(self, gravity, noise, bias, cov0=None, Rwb=None):
            self.g = np.array(gravity, D)
            self.noise = [f(x) for x in noise]
            self.bg, self.ba = np.array(bias[:3], np.float32).astype(D), np.array(bias[3:], np.float32).astype(D)
            self.dR, self.dv, self.dp, self.dt_total = I3.copy(), np.zeros(3, D), np.zeros(3, D), 0.0
            self.J = {k: np.zeros((3, 3), D) for k in ("R_bg", "v_bg", "v_ba", "p_bg", "p_ba")}
            self.cov = np.zeros((15, 15), D) if cov0 is None else np.array(cov0, np.float32).astype(D)
            self.Rwb = I3.copy() if Rwb is None else np.array(Rwb, np.float32).astype(D)
            self.prev, self.steps = None, 0

        def integrate(self, t, gyro, accel):
            m = (float(t), np.array(gyro, np.float32).astype(D), np.array(accel, np.float32).astype(D))
            if self.prev is None:
                self.prev = m
                return
            if m[0] <= self.prev[0]:
                return
            self.step(self.prev, m)
            self.prev = m

        def step(self, m0, m1):
            dt = m1[0] - m0[0]
            if dt < 1e-9:
                return
            h = f(np.float32(dt))  # static_cast<float>(dt) in either precision: the step length is an input
            w_mid = f(0.5) * ((m0[1] - self.bg) + (m1[1] - self.bg))
            a_mid = f(0.5) * ((m0[2] * f(1.0) - self.ba) + (m1[2] * f(1.0) - self.ba))
            phi, phi_h = w_mid * h, w_mid * (f(0.5) * h)
            R_step, R_half = q2r(so3_exp(phi)), q2r(so3_exp(phi_h))
            dR_mid = self.dR @ R_half
            J = dict(self.J)
            a_nav = dR_mid @ a_mid
            self.dR = self.dR @ R_step
            v_old = self.dv
            self.dp = self.dp + (v_old * h + f(0.5) * a_nav * h * h)
            self.dv = v_old + a_nav * h
            self.dt_total += dt
            Jr, Jrh, Sa = jr(phi), jr(phi_h), skew(a_mid)
            J_R_mid = R_half.T @ J["R_bg"] - Jrh * (f(0.5) * h)
            self.J["R_bg"] = R_step.T @ J["R_bg"] - Jr * h
            RSJ = dR_mid @ Sa @ J_R_mid
            self.J["v_bg"] = J["v_bg"] - RSJ * h
            self.J["v_ba"] = J["v_ba"] - dR_mid * h
            self.J["p_bg"] = J["p_bg"] + J["v_bg"] * h - f(0.5) * RSJ * h * h
            self.J["p_ba"] = J["p_ba"] + J["v_ba"] * h - f(0.5) * dR_mid * h * h
            has_noise = any(x > 0 for x in self.noise)
            if has_noise or not (np.abs(self.cov) <= 1e-5).all():
                F = np.eye(15, dtype=D)
                Rwm = self.Rwb @ dR_mid
                to_mid, bg_mid = R_half.T, -Jrh * (f(0.5) * h)
                F[0:3, 3:6] = f(-0.5) * Rwm @ Sa @ to_mid * h * h
                F[0:3, 6:9] = I3 * h
                F[0:3, 9:12] = f(-0.5) * Rwm * h * h
                F[0:3, 12:15] = f(-0.5) * Rwm @ Sa @ bg_mid * h * h
                F[3:6, 3:6] = R_step.T
                F[3:6, 12:15] = -Jr * h
                F[6:9, 3:6] = -Rwm @ Sa @ to_mid * h
                F[6:9, 9:12] = -Rwm * h
                F[6:9, 12:15] = -Rwm @ Sa @ bg_mid * h
                Q = np.zeros((15, 15), D)
                if has_noise:
                    sg, sa, sbg, sba = self.noise
                    h2 = h * h
                    h3 = h2 * h
                    G = np.zeros((15, 12), D)
                    G[0:3, 0:3] = f(-0.5) * Rwm * h2
                    G[6:9, 0:3] = -Rwm * h
                    G[3:6, 3:6] = -Jr * h
                    G[0:3, 3:6] = f(0.25) * Rwm @ Sa @ Jrh * h3
                    G[6:9, 3:6] = f(0.5) * Rwm @ Sa @ Jrh * h2
                    G[9:12, 6:9] = I3
                    G[12:15, 9:12] = I3
                    Qd = np.diag(np.repeat(np.array([sa * sa / h, sg * sg / h, sba * sba * h, sbg * sbg * h], D), 3)).astype(D)
                    Q = G @ Qd @ G.T
                P = F @ self.cov @ F.T + Q
                self.cov = np.where(np.eye(15, dtype=bool), P, (P + P.T) * f(0.5))
            self.steps += 1
            if self.steps % 100 == 0:
                self.dR = q2r(r2q(self.dR))

        def corrected(self, bias):
            d_bg = np.array(bias[:3], np.float32).astype(D) - self.bg
            d_ba = np.array(bias[3:], np.float32).astype(D) - self.ba
            dR = self.dR @ q2r(so3_exp(self.J["R_bg"] @ d_bg))
            q = r2q(dR)
            n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
            dR = q2r(q * (f(1.0) / n))
            return (dR, self.dv + (self.J["v_bg"] @ d_bg + self.J["v_ba"] @ d_ba),
                    self.dp + (self.J["p_bg"] @ d_bg + self.J["p_ba"] @ d_ba))

        def predict_relative(self, Rwb, v, bias):
            dR, _, dp = self.corrected(bias)
            h = f(np.float32(self.dt_total))
            Rt = np.array(Rwb, np.float32).astype(D).T
            free = dp + f(0.5) * (Rt @ self.g) * h * h
            return dR, free + Rt @ np.array(v, np.float32).astype(D) * h

    def trajectory(stamps, gyro, accel, start, duration, T_il, bias, gravity, Rwb, v, gyro_only):
        """imu_deskew.hpp:158-285 for a buffer that passes the coverage checks; (m, 8) in D"""
        end = start + duration
        keep = [i for i, t in enumerate(stamps) if start - 0.05 <= t <= end + 0.05]
        ts = [float(stamps[i]) for i in keep]
        g = [np.array(gyro[i], np.float32) for i in keep]
        a = [np.array(accel[i], np.float32) for i in keep]
        nxt = next((i for i, t in enumerate(ts) if t >= start), len(ts))
        assert 0 < nxt < len(ts)
        al = np.float32((start - ts[nxt - 1]) / (ts[nxt] - ts[nxt - 1]))
        # (std::fma in the reference: one rounding; the sample it gives is an input of both precisions, so round it once to float32)
        g0 = np.array([np.float32(np.float64(x1 - x0) * np.float64(al) + np.float64(x0)) for x0, x1 in zip(g[nxt - 1], g[nxt])])
        a0 = np.array([np.float32(np.float64(x1 - x0) * np.float64(al) + np.float64(x0)) for x0, x1 in zip(a[nxt - 1], a[nxt])])
        integ = Integ(gravity, (0, 0, 0, 0), bias)
        integ.integrate(start, g0, a0)
        T = np.array(T_il, np.float32).astype(D)
        Ti = np.eye(4, dtype=D)
        Ti[:3, :3] = T[:3, :3].T
        Ti[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
        out = [np.array([0, 0, 0, 1, 0, 0, 0, 0], D)]
        for i in range(nxt, len(ts)):
            integ.integrate(ts[i], g[i], a[i])
            t_rel = np.float32(ts[i] - start)
            if t_rel < 0:
                continue
            M = np.eye(4, dtype=D)
            if gyro_only:
                M[:3, :3] = integ.corrected(bias)[0]
            else:
                M[:3, :3], M[:3, 3] = integ.predict_relative(Rwb, v, bias)
            Tl = (T @ M) @ Ti
            out.append(np.r_[r2q(Tl[:3, :3]), Tl[:3, 3], f(t_rel)].astype(D))
        return np.array(out, D)

    ns = type("NS", (), {})
    ns.Integ, ns.trajectory = Integ, trajectory
    return ns


def imu_samples(rate_hz, t0, T, seed, gyro_amp=2.0):
    """float32 samples: gyro of up to gyro_amp rad/s per axis, specific force near gravity's reaction"""
    n = int(round(T * rate_hz))
    t = t0 + np.arange(n + 1) / rate_hz
    rs = np.random.RandomState(seed)
    ph = rs.uniform(0, 6.28, 6)
    gyro = np.stack([gyro_amp * np.sin(9.0 * t + ph[0]), 0.7 * gyro_amp * np.cos(13.0 * t + ph[1]),
                     gyro_amp * np.sin(5.0 * t + ph[2])], axis=1).astype(np.float32)
    accel = (np.array([0.3, -0.2, 9.8]) + np.stack([1.5 * np.sin(11.0 * t + ph[3]), 1.0 * np.cos(7.0 * t + ph[4]),
                                                     0.8 * np.sin(17.0 * t + ph[5])], axis=1)).astype(np.float32)
    return t, gyro, accel


BIAS_LIN = np.array([0.004, -0.003, 0.002, 0.03, -0.02, 0.05], np.float32)
BIAS_NEW = BIAS_LIN + np.array([0.001, -0.0015, 0.0008, 0.004, 0.002, -0.003], np.float32)
NOISE = (1e-3, 1e-2, 1e-5, 1e-4)  # gyro, accel, gyro bias random walk, accel bias random walk
P0_DIAG = np.diag(np.repeat([1e-4, 1e-6, 1e-4, 1e-8, 1e-8], 3)).astype(np.float32)


@pytest.mark.parametrize("rate_hz", [200, 1000])
@pytest.mark.parametrize("noise", ["noise", "no-noise"])
def test_integrator_against_float64(L, api, rate_hz, noise):
    """sp_imu_preint_* against the float64 evaluation: E_lib <= 4 * E_ref per quantity, over a window of more than 100 steps at
    1 kHz (the renormalisation fires), with one duplicate stamp (dropped), a non-zero linearisation bias and a changed bias estimate."""
    t, gyro, accel = imu_samples(rate_hz, 10.0, 0.14, seed=rate_hz)
    dup = len(t) // 3
    t, gyro, accel = np.insert(t, dup, t[dup - 1]), np.insert(gyro, dup, gyro[dup] + 1.0, axis=0), np.insert(accel, dup, accel[dup], axis=0)
    Rwb = rot_z(0.7)
    nz = NOISE if noise == "noise" else (0.0, 0.0, 0.0, 0.0)
    lib = api.IMUPreintegration(api.IMUPreintegrationParams(GRAVITY, 1.0, *nz))
    lib.reset(BIAS_LIN, P0_DIAG, Rwb)
    ref = {}
    for D in (np.float32, np.float64):
        it = np_integrator(D).Integ(GRAVITY, nz, BIAS_LIN, P0_DIAG, Rwb)
        ref[D] = it
    for ti, g, a in zip(t, gyro, accel):
        lib.integrate(ti, g, a)
        for it in ref.values():
            it.integrate(ti, g, a)
    assert ref[np.float64].steps == len(t) - 2 and (rate_hz < 1000 or ref[np.float64].steps > 100)
    raw, cor = lib.get_raw(), lib.get_corrected(BIAS_NEW)
    assert raw.dt_total == ref[np.float64].dt_total
    got = dict(Delta_R=raw.Delta_R, Delta_v=raw.Delta_v, Delta_p=raw.Delta_p, J_R_bg=raw.J_R_bg, J_v_bg=raw.J_v_bg, J_v_ba=raw.J_v_ba,
               J_p_bg=raw.J_p_bg, J_p_ba=raw.J_p_ba, covariance=raw.covariance, corrected_R=cor.Delta_R, corrected_v=cor.Delta_v,
               corrected_p=cor.Delta_p)

    def quantities(it):
        c = it.corrected(BIAS_NEW)
        return dict(Delta_R=it.dR, Delta_v=it.dv, Delta_p=it.dp, J_R_bg=it.J["R_bg"], J_v_bg=it.J["v_bg"], J_v_ba=it.J["v_ba"],
                    J_p_bg=it.J["p_bg"], J_p_ba=it.J["p_ba"], covariance=it.cov, corrected_R=c[0], corrected_v=c[1], corrected_p=c[2])

    q32, q64 = quantities(ref[np.float32]), quantities(ref[np.float64])
    assert all(v.dtype == np.float32 for v in q32.values())  # the transcription stayed in float32
    bad = []
    for k in got:
        E_ref = float(np.abs(q32[k].astype(np.float64) - q64[k]).max())
        E_lib = float(np.abs(got[k].astype(np.float64) - q64[k]).max())
        print(f"integrator [{rate_hz:4d} Hz {noise:8s}] {k:12s}: E_lib = {E_lib:.3e}  E_ref = {E_ref:.3e}  bound 4")
        if not E_lib <= 4.0 * E_ref:
            bad.append((k, E_lib, E_ref))
    assert not bad, bad
    if noise == "no-noise":  # (and with nothing to propagate the covariance stays exactly zero: the step is skipped)
        lib.reset(BIAS_LIN)
        for ti, g, a in zip(t, gyro, accel):
            lib.integrate(ti, g, a)
        assert not lib.get_raw().covariance.any()


@pytest.mark.parametrize("rate_hz", [200, 1000])
@pytest.mark.parametrize("gyro_only", [False, True])
def test_trajectory_against_float64(L, rate_hz, gyro_only):
    """sp_imu_deskew_trajectory_host against the float64 evaluation, E_lib <= 4 * E_ref for the quaternions and the translations;
    the stamps are equal bit for bit. A 0.1 s scan that starts between two samples, an extrinsic with a lever arm, a start
    velocity."""
    t, gyro, accel = imu_samples(rate_hz, 19.96, 0.2, seed=7 + rate_hz)
    start, duration = 20.0 + 0.37 / rate_hz, 0.1
    T_il = np.eye(4, dtype=np.float32)
    T_il[:3, :3] = rot_z(0.3) @ np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
    T_il[:3, 3] = [0.1, -0.05, 0.2]
    Rwb, v = rot_z(-0.4), np.array([3.0, -1.0, 0.2], np.float32)
    rc, st, traj = c_trajectory(L, t, gyro, accel, start, duration, gyro_only=gyro_only, bias=BIAS_LIN, T_il=T_il, Rwb=Rwb, v=v)
    assert (rc, st) == (0, 0)
    r32 = np_integrator(np.float32).trajectory(t, gyro, accel, start, duration, T_il, BIAS_LIN, GRAVITY, Rwb, v, gyro_only)
    r64 = np_integrator(np.float64).trajectory(t, gyro, accel, start, duration, T_il, BIAS_LIN, GRAVITY, Rwb, v, gyro_only)
    assert r32.dtype == np.float32 and traj.shape == r64.shape and traj.shape[0] >= int(0.1 * rate_hz)
    assert np.array_equal(traj[:, 7], r64[:, 7].astype(np.float32))
    bad = []
    for name, sl in (("q", slice(0, 4)), ("t", slice(4, 7))):
        E_ref = float(np.abs(r32[:, sl].astype(np.float64) - r64[:, sl]).max())
        E_lib = float(np.abs(traj[:, sl].astype(np.float64) - r64[:, sl]).max())
        print(f"trajectory [{rate_hz:4d} Hz gyro_only={gyro_only}] {name}: E_lib = {E_lib:.3e}  E_ref = {E_ref:.3e}  bound 4")
        if not E_lib <= 4.0 * E_ref:
            bad.append((name, E_lib, E_ref))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ intervals, the restatement
def lib_intervals(L, traj):
    rows = np.full((len(traj) - 1, 16), 5.0, np.float32)
    assert L.sp_imu_deskew_intervals_host(_ptr(np.ascontiguousarray(traj, np.float32)), len(traj), _ptr(rows)) == 0
    return rows


def test_intervals_bit_identical_to_per_point_slerp(L, R):
    for n_traj, rate, seed in ((2, 1.5, 1), (26, 1.5, 2), (300, 0.2, 3), (300, 0.01, 4), (26, 30.0, 5)):
        traj = synthetic_trajectory(n_traj, rate, 3.0, seed=seed)
        if n_traj == 26:  # a pose on the far side of the sphere: the logarithm sees -q1
            traj[7, :4] *= -1.0
        rows = lib_intervals(L, traj)
        want, q1s = np.empty_like(rows), np.empty((n_traj - 1, 4), np.float32)
        R.imu_intervals_restate(_ptr(traj), n_traj, _ptr(want), _ptr(q1s))
        assert np.array_equal(rows.view(np.uint32), want.view(np.uint32)), n_traj
        assert np.array_equal(rows[:, 2:6].view(np.uint32), traj[:-1, :4].view(np.uint32))  # q0 as it is
        flip = np.einsum("ij,ij->i", traj[:-1, :4].astype(np.float64), traj[1:, :4].astype(np.float64)) < 0
        assert np.array_equal(q1s, np.where(flip[:, None], -traj[1:, :4], traj[1:, :4]))
        if n_traj == 26:
            assert flip.any()
        assert not rows[:, 15].any()


def test_exact_properties(R):
    n = 4000
    pts, covs, nrm = random_cloud(n, seed=7)
    rs = np.random.RandomState(1)
    pts[:, 3] = rs.choice([1.0, 0.0, 2.5], n).astype(np.float32)  # w is carried, whatever it is
    for n_traj, rate, acc in ((26, 1.5, 3.0), (3, 0.2, 0.5), (300, 0.01, 0.0), (2, 1.5, 3.0)):
        traj = synthetic_trajectory(n_traj, rate, acc)
        last_ms = np.float32(100.0)
        assert np.float32(last_ms * np.float32(1e-3)) >= traj[-1, 7]
        # t = 0: point, normal and the 3x3 covariance bit-identical; normal w and the covariance's fourth row / column are 0
        po, co, no = restate(R, pts, covs, nrm, np.zeros(n, np.float32), traj)
        assert np.array_equal(po.view(np.uint32), pts.view(np.uint32))
        assert np.array_equal(no[:, :3].view(np.uint32), nrm[:, :3].view(np.uint32)) and not no[:, 3].any()
        c4, i4 = co.reshape(n, 4, 4), covs.reshape(n, 4, 4)
        assert np.array_equal(c4[:, :3, :3].view(np.uint32), i4[:, :3, :3].view(np.uint32))
        assert not c4[:, 3, :].any() and not c4[:, :, 3].any()
        # t < 0 equals t = 0; t past the last stamp equals t on it
        neg = restate(R, pts, covs, nrm, np.full(n, -3.0, np.float32), traj)
        full = restate(R, pts, covs, nrm, np.full(n, last_ms, np.float32), traj)
        over = restate(R, pts, covs, nrm, np.full(n, 250.0, np.float32), traj)
        for a, b in zip(neg, (po, co, no)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        for a, b in zip(over, full):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # a non-finite time stamp: every row bit-identical, the covariance's fourth row and column included
        for bad in (np.nan, np.inf, -np.inf):
            cp = restate(R, pts, covs, nrm, np.full(n, bad, np.float32), traj)
            for a, b in zip(cp, (pts, covs, nrm)):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # anywhere in between: w is the input's, normal w and the covariance's fourth row / column are exactly 0
        tm = rs.uniform(0, 100, n).astype(np.float32)
        pm, cm, nm = restate(R, pts, covs, nrm, tm, traj)
        assert np.array_equal(pm[:, 3].view(np.uint32), pts[:, 3].view(np.uint32))
        assert not nm[:, 3].any()
        cm4 = cm.reshape(n, 4, 4)
        assert not cm4[:, 3, :].any() and not cm4[:, :, 3].any()
        assert not np.array_equal(pm[:, :3], pts[:, :3])
        # the attribute sets do not influence each other, and in place is out of place
        assert np.array_equal(restate(R, pts, None, None, tm, traj)[0].view(np.uint32), pm.view(np.uint32))
        ip = restate(R, pts, covs, nrm, tm, traj, in_place=True)
        for a, b in zip(ip, (pm, cm, nm)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # equal neighbouring stamps: alpha = 0, so a point stamped there gets the interval's first pose exactly
    traj = synthetic_trajectory(26, 1.5, 3.0)
    k = 26 // 2
    assert traj[k, 7] == traj[k - 1, 7]
    two = np.stack([traj[k], traj[k]])  # an interval of zero length on its own: every stamp maps to pose k
    t_eq = np.full(n, traj[k, 7] * 1e3, np.float32)
    sel = np.float32(t_eq * np.float32(1e-3)) == traj[k, 7]
    assert sel.all()
    a = restate(R, pts, covs, nrm, t_eq, traj)
    b = restate(R, pts, covs, nrm, t_eq, two)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_restatement_against_float64(R):
    """The float32 restatement stays within float32 rounding of the float64 evaluation of the same formula (the yardstick the GPU
    suite measures the device with): positions of up to 87 m, so 1e-4 absolute is ~15 ulp of the largest coordinate."""
    n = 20000
    pts, covs, nrm = random_cloud(n, seed=11)
    tm = np.random.RandomState(2).uniform(-5, 110, n).astype(np.float32)
    for n_traj, rate, acc in ((26, 1.5, 3.0), (300, 0.2, 0.5), (5000, 0.01, 0.0)):
        traj = synthetic_trajectory(n_traj, rate, acc)
        a = restate(R, pts, covs, nrm, tm, traj)
        b = restate(R, pts, covs, nrm, tm, traj, f64=True)
        assert np.abs(a[0] - b[0]).max() <= 1e-4
        assert np.abs(a[2] - b[2]).max() <= 1e-6
        assert np.abs(a[1] - b[1]).max() <= 1e-6 * np.abs(b[1]).max()
