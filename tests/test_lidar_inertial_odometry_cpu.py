"""Host numerics of the LiDAR-inertial odometry loop (the last section of csrc/lio_host.hip) through sycl_points_amd.api against
float64 numpy models written here, and the host-only C++ program of the facade (tests/cpp/test_lidar_inertial_odometry_host.cpp).
No GPU.

Bounds:
  predict_state      as tests/test_lidar_odometry_cpu.py: 1e-5 absolute for rotation entries, 1e-5 * max(1, |x|) for positions and
                     velocities (three rigid products and one 3x3 product: a few dozen float32 roundings of 6e-8 each on entries <= 10).
  reset_covariance   the bound tests/test_lio_cpu.py applies to cov_lidar_to_imu: error <= 4 K eps32 scale over all entries and 8
                     seeds, scale = max|J^-1|^2 max|P_in|, K = max(1, K_ref), K_ref the worst error / (eps32 scale) of the SAME
                     formulas (tests/f64_lio.py) run in numpy float32, never measured on the library. The way back (imu -> lidar
                     of the output recovers P_post + floors) under that file's round_trip bound, the roles of J and J^-1
                     exchanged: scale = max|J|^2 max|P_imu|.
  bias_observable    exact: the edge cases are built so that float32 computes the deviation without rounding (samples +-d about
                     an exactly representable mean; sqrt(fl(d * d)) == d in binary floating point).
  clamp              |norm - max_norm| <= 4 ulp(max_norm), the direction within 4 eps32.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import f64_lio as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = M.EPS32
ROT_TOL = 1e-5
G = 9.80665
SEEDS = list(range(8))
NEW_SYMBOLS = ["sp_lio_bias_observable_host", "sp_lio_clamp_bias_host", "sp_lio_predict_state_host", "sp_lio_reset_covariance_host"]
f32 = np.float32


@pytest.fixture(scope="module")
def sp():
    from sycl_points_amd import _lib

    _lib.build()
    import sycl_points_amd.api as api

    return api


def trans_tol(t):
    return 1e-5 * max(1.0, float(np.abs(t).max()))


def random_rotation(rs, lo, hi):
    axis = rs.normal(size=3)
    return M.rodrigues(axis / np.linalg.norm(axis) * rs.uniform(lo, hi))


def extrinsic(rs):
    """a rotation of 0.1 to 0.6 rad and a lever arm of 10 to 30 cm, float32 (the extrinsic of tests/test_lio_cpu.py's cases)"""
    T = np.eye(4)
    T[:3, :3] = random_rotation(rs, 0.1, 0.6)
    lever = rs.normal(size=3)
    T[:3, 3] = lever / np.linalg.norm(lever) * rs.uniform(0.10, 0.30)
    return T.astype(f32)


def isometry_inverse(T):
    Ti = np.eye(4, dtype=T.dtype)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return Ti


# ------------------------------------------------------------------------------------------------------------- ABI
def test_abi_is_additive(sp):
    from sycl_points_amd import _lib

    header = open(os.path.join(ROOT, "include", "sycl_points_amd.h")).read()
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.lib().sp_abi_version() == 7
    # null arguments are refused before anything is read
    L = _lib.lib()
    assert L.sp_lio_clamp_bias_host(None, 1.0) == _lib.SP_ERR_INVALID_ARGUMENT
    assert L.sp_lio_predict_state_host(None, None, None, None, 0.1, None, None) == _lib.SP_ERR_INVALID_ARGUMENT
    assert L.sp_lio_reset_covariance_host(None, 0.1, 0.01, None, None, None, None) == _lib.SP_ERR_INVALID_ARGUMENT
    assert L.sp_lio_bias_observable_host(None, None, 5, 1, 0.03, 0.3, None) == _lib.SP_ERR_INVALID_ARGUMENT
    out = C.c_int(-1)
    assert L.sp_lio_bias_observable_host(None, None, 5, 1, 0.03, 0.3, C.byref(out)) == _lib.SP_ERR_INVALID_ARGUMENT
    P = np.zeros(225, f32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    T, R = np.eye(4, dtype=f32).reshape(-1), np.eye(3, dtype=f32).reshape(-1)
    assert L.sp_lio_reset_covariance_host(vp(P), 0.1, 0.01, vp(T), vp(R), vp(P), vp(R.copy())) == _lib.SP_ERR_INVALID_ARGUMENT  # in place


# ------------------------------------------------------------------------------------------------------------- predict_state
def predict_model(x, T_i2l, T_rel, dv, dt, g):
    """lidar_inertial_odometry.hpp:432-459 in float64 on the float32 inputs"""
    T_i2l, T_rel = np.asarray(T_i2l, np.float64), np.asarray(T_rel, np.float64)
    T_pred = x.pose() @ (T_i2l @ T_rel @ isometry_inverse(T_i2l))
    v = x.v + np.asarray(g, np.float64) * float(dt) + (x.R @ T_i2l[:3, :3]) @ np.asarray(dv, np.float64)
    return M.St(T_pred[:3, 3], T_pred[:3, :3], v, x.ba, x.bg)


def random_state(rs):
    return M.St(rs.uniform(-8, 8, 3), random_rotation(rs, 0.2, 2.5), rs.uniform(-3, 3, 3), rs.uniform(-0.1, 0.1, 3), rs.uniform(-0.01, 0.01, 3), f32)


@pytest.mark.parametrize("seed", SEEDS)
def test_predict_state_against_float64(sp, seed):
    rs = np.random.RandomState(2000 + seed)
    x32 = random_state(rs)
    T_i2l = extrinsic(rs)
    lever = np.linalg.norm(T_i2l[:3, 3])
    assert 0.10 <= lever <= 0.30 and not np.allclose(T_i2l[:3, :3], np.eye(3), atol=0.05)
    T_rel = np.eye(4)
    T_rel[:3, :3] = random_rotation(rs, 0.01, 0.2)
    T_rel[:3, 3] = rs.uniform(-0.5, 0.5, 3)
    T_rel = T_rel.astype(f32)
    dv = rs.uniform(-1.0, 1.0, 3).astype(f32)
    dt = f32(rs.uniform(0.05, 0.2))
    g = np.array([0.0, 0.0, -G], f32)
    assert np.abs(dv).min() > 0 and np.abs(x32.v).min() > 0
    got = sp.lio_predict_state(sp.IMUState.unpack(x32.pack()), T_i2l, T_rel, dv, float(dt), g)
    x64 = M.St.unpack(x32.pack().astype(np.float64))
    want = predict_model(x64, T_i2l, T_rel, dv, dt, g)
    err_R = np.abs(got.rotation - want.R).max()
    err_p = np.abs(got.position - want.p).max()
    err_v = np.abs(got.velocity - want.v).max()
    print(f"[lio-predict] seed {seed}: rotation {err_R:.3g} (bound {ROT_TOL}), position {err_p:.3g} ({trans_tol(want.p):.3g}), "
          f"velocity {err_v:.3g} ({trans_tol(want.v):.3g})")
    assert np.abs(want.p).max() <= 10.0 and np.abs(want.v).max() <= 10.0
    assert err_R <= ROT_TOL
    assert err_p <= trans_tol(want.p)
    assert err_v <= trans_tol(want.v)
    assert np.array_equal(got.accel_bias, x32.ba) and np.array_equal(got.gyro_bias, x32.bg)  # copied
    # each term matters at this bound: the prediction without the extrinsic, the gravity term or Delta_v is off by far more
    for broken in (predict_model(x64, np.eye(4), T_rel, dv, dt, g), predict_model(x64, T_i2l, T_rel, dv, dt, 0 * g),
                   predict_model(x64, T_i2l, T_rel, 0 * dv, dt, g)):
        assert max(np.abs(broken.p - want.p).max(), np.abs(broken.v - want.v).max()) > 1e-3


def test_predict_state_identity_returns_the_state_bit_for_bit(sp):
    rs = np.random.RandomState(7)
    x = random_state(rs)
    got = sp.lio_predict_state(sp.IMUState.unpack(x.pack()), np.eye(4), np.eye(4), np.zeros(3), 0.0, [0.0, 0.0, -G])
    assert np.array_equal(got.pack().view(np.uint32), x.pack().astype(f32).view(np.uint32))
    # zero motion over a non-zero interval from rest: gravity alone changes the velocity
    got = sp.lio_predict_state(sp.IMUState.unpack(x.pack()), np.eye(4), np.eye(4), np.zeros(3), 0.1, [0.0, 0.0, -G])
    assert np.array_equal(got.position, x.p) and np.array_equal(got.rotation, x.R)
    assert np.array_equal(got.velocity, (x.v + np.array([0, 0, -G], f32) * f32(0.1)).astype(f32))


# ------------------------------------------------------------------------------------------------------------- reset_covariance
def spd(rs, scale):
    Q, _ = np.linalg.qr(rs.normal(size=(15, 15)))
    P = (Q * rs.uniform(1.0, 4.0, 15)) @ Q.T * scale
    return ((P + P.T) / 2).astype(f32)


def floors(P, sv, sr, dt):
    """P + sv^2 I on the velocity block + sr^2 I on the rotation block, in precision dt (lidar_inertial_odometry.hpp:412-417)"""
    out = P.astype(dt).copy()
    sv2, sr2 = dt(sv) * dt(sv), dt(sr) * dt(sr)
    for i in range(3):
        out[M.VEL + i, M.VEL + i] += sv2
        out[M.ROT + i, M.ROT + i] += sr2
    return out


def reset_case(seed):
    rs = np.random.RandomState(3000 + seed)
    return dict(P=spd(rs, 1e-3), T=extrinsic(rs), R=random_rotation(rs, 0.2, 2.5).astype(f32), sv=f32(0.1), sr=f32(0.01))


def reset_model(c, dt):
    """-> P_initial_imu, R_world_imu, and the way back to the LiDAR error state, all in precision dt"""
    T, R = c["T"].astype(dt), c["R"].astype(dt)
    Pin = floors(c["P"], c["sv"], c["sr"], dt)
    Pimu = M.transform_covariance(Pin, T, R, 1)
    return Pin, Pimu, R @ T[:3, :3], M.transform_covariance(Pimu, T, R, 0)


def test_reset_covariance_against_float64(sp):
    worst = {"cov": 0.0, "back": 0.0}
    kref = {"cov": 0.0, "back": 0.0}
    rows = []
    for seed in SEEDS:
        c = reset_case(seed)
        Pin, Pimu, Rwi, back = reset_model(c, np.float64)
        _, Pimu32, _, back32 = reset_model(c, f32)
        Ji = M.jacobian(c["T"].astype(np.float64), c["R"].astype(np.float64), inverse=True)
        J = M.jacobian(c["T"].astype(np.float64), c["R"].astype(np.float64))
        scale_cov = float(np.abs(Ji).max() ** 2 * np.abs(Pin).max())
        scale_back = float(np.abs(J).max() ** 2 * np.abs(Pimu).max())
        kref["cov"] = max(kref["cov"], np.abs(Pimu32.astype(np.float64) - Pimu).max() / (EPS * scale_cov))
        kref["back"] = max(kref["back"], np.abs(back32.astype(np.float64) - Pin).max() / (EPS * scale_back))
        # the model's own way back is P_post + floors as far as the float32 extrinsic rotation is orthonormal
        assert np.abs(back - Pin).max() <= EPS * np.abs(Pin).max()
        got_P, got_R = sp.lio_reset_covariance(c["P"], float(c["sv"]), float(c["sr"]), c["T"], c["R"])
        got_back = sp.transform_covariance_imu_to_lidar(got_P, c["T"], c["R"])
        rows.append((np.abs(got_P.astype(np.float64) - Pimu).max() / (EPS * scale_cov),
                     np.abs(got_back.astype(np.float64) - Pin).max() / (EPS * scale_back)))
        worst["cov"], worst["back"] = max(worst["cov"], rows[-1][0]), max(worst["back"], rows[-1][1])
        assert np.abs(got_R - Rwi).max() <= ROT_TOL
        # the floors are in: without them the velocity block would be smaller by sv^2 = 1e-2, ten times the covariance itself
        assert np.abs(got_P[M.VEL:M.VEL + 3, M.VEL:M.VEL + 3] - c["P"][M.VEL:M.VEL + 3, M.VEL:M.VEL + 3]).max() > 5e-3
    print("\n[lio-reset] worst error / (eps32 scale): quantity, numpy float32 (K_ref), library")
    for name in worst:
        print(f"[lio-reset]   {name:6s} {kref[name]:8.3f} {worst[name]:8.3f}")
    for name in worst:
        assert worst[name] <= 4 * max(1.0, kref[name]), (name, worst[name], kref[name])


@pytest.mark.parametrize("seed", SEEDS[:3])
def test_reset_covariance_without_floors_is_the_transform_bit_for_bit(sp, seed):
    c = reset_case(seed)
    got_P, got_R = sp.lio_reset_covariance(c["P"], 0.0, 0.0, c["T"], c["R"])
    want = sp.transform_covariance_lidar_to_imu(c["P"], c["T"], c["R"])
    assert np.array_equal(got_P.view(np.uint32), want.view(np.uint32))
    # ... and with them it is the transform of P + floors, bit for bit: one copy of the code
    got_P, _ = sp.lio_reset_covariance(c["P"], float(c["sv"]), float(c["sr"]), c["T"], c["R"])
    want = sp.transform_covariance_lidar_to_imu(floors(c["P"], c["sv"], c["sr"], f32), c["T"], c["R"])
    assert np.array_equal(got_P.view(np.uint32), want.view(np.uint32))
    # R_world_imu = R R_i2l in float32, the products summed in index order
    R, Ri = c["R"], c["T"][:3, :3]
    want_R = np.zeros((3, 3), f32)
    for i in range(3):
        for j in range(3):
            s = f32(0)
            for k in range(3):
                s = f32(s + f32(R[i, k] * Ri[k, j]))
            want_R[i, j] = s
    assert np.array_equal(got_R, want_R)


# ------------------------------------------------------------------------------------------------------------- bias_observable
def window(n, gyro_dev=0.0, accel_dev=0.0):
    """n (a power of two) samples +-dev about gyro (0, 0, 0.25) and accel (0, 0, G): the float32 means are exact, so the float32
    deviation is |dev| exactly"""
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(f32)
    gyro = np.tile(np.array([0.0, 0.0, 0.25], f32), (n, 1))
    accel = np.tile(np.array([0.0, 0.0, G], f32), (n, 1))
    gyro[:, 0] = sign * f32(gyro_dev)
    accel[:, 1] = sign * f32(accel_dev)
    return gyro, accel


def test_bias_observable_freeze_off_and_short_windows(sp):
    gyro, accel = window(4)
    assert sp.lio_bias_observable(gyro, accel, freeze_on_low_excitation=False) is True  # at rest, yet never frozen
    assert sp.lio_bias_observable(np.zeros((0, 3)), np.zeros((0, 3)), freeze_on_low_excitation=False) is True
    big_g, big_a = window(4, 1.0, 5.0)
    for n in (0, 1):  # fewer than two samples: not observable, whatever the one sample says
        assert sp.lio_bias_observable(big_g[:n], big_a[:n], freeze_on_low_excitation=True) is False
    assert sp.lio_bias_observable(big_g[:2], big_a[:2], freeze_on_low_excitation=True) is True
    assert sp.lio_bias_observable(gyro, accel, freeze_on_low_excitation=True) is False  # at rest


@pytest.mark.parametrize("which,threshold", [("gyro", 0.03), ("accel", 0.3)])
def test_bias_observable_threshold_edges(sp, which, threshold):
    """just below, exactly at (strict >: 0) and just above each threshold, the other sensor at rest"""
    thr = f32(threshold)
    below, above = np.nextafter(thr, f32(0)), np.nextafter(thr, f32(1))
    for dev, want in ((below, False), (thr, False), (above, True)):
        gyro, accel = window(4, **{f"{which}_dev": dev})
        assert sp.lio_bias_observable(gyro, accel, True, 0.03, 0.3) is want, (which, float(dev))
    # the thresholds are arguments: the same windows against a threshold one float32 lower
    gyro, accel = window(4, **{f"{which}_dev": thr})
    kw = dict(gyro_excitation_threshold=0.03, accel_excitation_threshold=0.3)
    kw[f"{which}_excitation_threshold"] = float(below)
    assert sp.lio_bias_observable(gyro, accel, True, **kw) is True
    # the deviation is the norm of the full vector: 0.8 thr on two axes is 1.13 thr
    gyro, accel = window(4)
    arr = gyro if which == "gyro" else accel
    sign = np.where(np.arange(4) % 2 == 0, 1.0, -1.0).astype(f32)
    arr[:, 0] = sign * f32(0.8) * thr
    arr[:, 1] = sign * f32(0.8) * thr
    assert sp.lio_bias_observable(gyro, accel, True, 0.03, 0.3) is True


def test_bias_observable_constant_rate_turn(sp):
    """the case the reference's comment names: the gyro is constant, |a| is constant, the direction of a sweeps"""
    n = 21
    phi = np.linspace(0.0, 0.1, n)  # 0.5 rad/s over 0.2 s
    gyro = np.tile(np.array([0.0, 0.5, 0.0], f32), (n, 1))
    accel = (G * np.stack([np.sin(phi), np.zeros(n), np.cos(phi)], 1)).astype(f32)
    a64 = accel.astype(np.float64)
    norms = np.linalg.norm(a64, axis=1)
    sweep = np.linalg.norm(a64 - a64.mean(0), axis=1).max()
    print(f"[lio-bias] turn: max |a - mean a| = {sweep:.4f}, max ||a| - mean |a|| = {np.abs(norms - norms.mean()).max():.2e}")
    assert sweep > 0.3 * 1.5 and np.abs(norms - norms.mean()).max() < 1e-5  # the magnitude alone would see nothing
    assert np.abs(gyro.astype(np.float64) - gyro.astype(np.float64).mean(0)).max() == 0.0
    assert sp.lio_bias_observable(gyro, accel, True, 0.03, 0.3) is True
    assert sp.lio_bias_observable(gyro, np.tile(accel[:1], (n, 1)), True, 0.03, 0.3) is False  # the same window without the sweep


@pytest.mark.parametrize("seed", SEEDS)
def test_bias_observable_against_float64(sp, seed):
    """random windows whose float64 deviations are at least 1 % away from both thresholds"""
    rs = np.random.RandomState(4000 + seed)
    n = int(rs.randint(5, 40))
    gyro = (rs.normal(0, 1, 3) * 0.2 + rs.normal(0, 1, (n, 3)) * rs.choice([0.002, 0.02])).astype(f32)
    accel = (np.array([0, 0, G]) + rs.normal(0, 1, (n, 3)) * rs.choice([0.02, 0.2])).astype(f32)
    dev = lambda a: np.linalg.norm(a.astype(np.float64) - a.astype(np.float64).mean(0), axis=1).max()  # noqa: E731
    dg, da = dev(gyro), dev(accel)
    assert abs(dg / 0.03 - 1) > 0.01 and abs(da / 0.3 - 1) > 0.01
    assert sp.lio_bias_observable(gyro, accel, True, 0.03, 0.3) is bool(dg > 0.03 or da > 0.3)


# ------------------------------------------------------------------------------------------------------------- clamp
def test_clamp_bias(sp):
    rs = np.random.RandomState(11)
    for _ in range(50):
        b = (rs.normal(size=3) * rs.choice([1e-3, 0.05, 2.0])).astype(f32)
        norm = float(np.linalg.norm(b.astype(np.float64)))
        for disabled in (0.0, -1.0):  # no-op, bit for bit
            assert np.array_equal(sp.lio_clamp_bias(b, disabled).view(np.uint32), b.view(np.uint32))
        roomy = sp.lio_clamp_bias(b, norm * 1.5)  # shorter than the limit: no-op
        assert np.array_equal(roomy.view(np.uint32), b.view(np.uint32))
        limit = f32(norm * rs.uniform(0.05, 0.9))
        got = sp.lio_clamp_bias(b, float(limit))
        got_norm = float(np.linalg.norm(got.astype(np.float64)))
        assert abs(got_norm - float(limit)) <= 4 * float(np.spacing(limit)), (got_norm, limit)
        direction = got.astype(np.float64) / got_norm - b.astype(np.float64) / norm
        assert np.abs(direction).max() <= 4 * EPS
    # exactly at the limit: kept (the comparison is strict)
    b = np.array([0.0, 0.5, 0.0], f32)
    assert np.array_equal(sp.lio_clamp_bias(b, 0.5), b)
    assert np.array_equal(sp.lio_clamp_bias(b, 0.25), np.array([0.0, 0.25, 0.0], f32))


# ------------------------------------------------------------------------------------------------------------- the facade
def cxx(*args, **kw):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    return subprocess.run(["g++", "-O2", "-std=c++20", f"-I{ROOT}/include", f"-I{rocm}/include", "-D__HIP_PLATFORM_AMD__", "-Wall",
                           "-Wno-unused-value", "-Wno-unused-result", *args], capture_output=True, text=True, **kw)


@pytest.mark.parametrize("header", ["sycl_points/pipeline/lidar_inertial_odometry.hpp", "sycl_points/pipeline/lidar_inertial_odometry_params.hpp"])
def test_forwarding_header_compiles_on_its_own(header):
    """a translation unit of that one include, at the reference's path, naming the reference's types"""
    unit = (f'#include "{header}"\n'
            "using P = sycl_points::pipeline::lidar_inertial_odometry::Parameters;\n"
            "static_assert(sizeof(P::LIO::BiasEstimation) > 0 && sizeof(P::LIO::PreintegrationReset) > 0);\n")
    if not header.endswith("_params.hpp"):
        unit += "using L = sycl_points::pipeline::lidar_inertial_odometry::LidarInertialOdometryPipeline;\nstatic_assert(sizeof(L::Ptr) > 0);\n"
    r = cxx("-fsyntax-only", "-x", "c++", "-", input=unit)
    assert r.returncode == 0, r.stderr[-4000:]


def test_host_cpp_program(tmp_path):
    """tests/cpp/test_lidar_inertial_odometry_host.cpp with tests/cpp/Makefile's flags (the Makefile is not changed): the types at
    the reference's names, every default of the LIO block, the ResultType values. No device is touched."""
    from sycl_points_amd import _lib

    _lib.build()
    exe = str(tmp_path / "test_lidar_inertial_odometry_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.join(ROOT, "sycl_points_amd", "lib")
    b = cxx(os.path.join(ROOT, "tests", "cpp", "test_lidar_inertial_odometry_host.cpp"), "-o", exe, f"-L{libdir}", "-lsycl_points_amd",
            f"-Wl,-rpath,{libdir}", f"-L{rocm}/lib", "-lamdhip64", f"-Wl,-rpath,{rocm}/lib")
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-6000:], r.stderr[-3000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failed" in r.stdout
    for name in ("types_at_the_reference_names", "lio_block_defaults", "result_type_values"):
        assert f"[  OK  ] {name}" in r.stdout, name
