"""IMU deskew on the device (sp_deskew_imu, api.deskew_point_cloud_imu and, through tests/cpp/test_imu.cpp, the C++ facade's
imu::IMUPreintegration / deskew::deskew_point_cloud_imu) against the CPU restatement of the reference kernel
(tests/cpp/imu_deskew_restate.cpp; deskew/imu_deskew.hpp:330-411), which evaluates the slerp per point as the reference writes it.

The exact properties of the restatement (tests/test_imu_cpu.py) hold bit for bit on the device; so does every row whose stamp lies
exactly on a pose of the trajectory (alpha = 0: so3_exp takes its polynomial branch, no sinf / cosf is evaluated, and the rest is
fma chains). Everything else is measured with a float64 evaluation of the same formula as the yardstick: E_ref is the restatement's
largest absolute error against it, E_dev the device's, per attribute, trajectory and motion, and the device passes when
E_dev <= m * E_ref with tests/test_gpu_deskew.py's m: the restatement's sinf / cosf are glibc's (1 ulp), OpenCL's bound for the
device's is 4 ulp, m = 4 / 1 * 2 = 8, the 2 for the spread between two samples' worst rows. The device functions are the same.

m, E_ref and E_dev are printed for every case before the assertion (run with -s). Measured figures: none yet — no MI355X could be
reached when this file was written.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
K_BLOCK, FULL_GRID = 256, 256 * 8  # csrc/sp_common.h: kBlock, and stream_grid's cap of 8 workgroups on each of 256 CUs
N = FULL_GRID * K_BLOCK + 293      # one full grid-stride trip, a second partial one, a ragged tail: 524 581 points
SMALL = (1, 63, 65, 257)
M_BOUND = 8.0  # (4 ulp device sinf / cosf over 1 ulp glibc) x 2
MOTIONS = {"fast": (1.5, 3.0), "slow": (0.2, 0.5), "crawl": (0.01, 0.0)}  # rad/s, m/s^2 over a 0.1 s scan
N_TRAJ = (2, 3, 26, 300, 5000)  # no bisection | one step | 200 Hz | more rows than a workgroup has lanes | beyond the LDS bound
ATTRS = {"points": (False, False), "points+covs": (True, False), "points+normals": (False, True), "all": (True, True)}
GROUPS = ("zero", "neg", "over", "on_stamp", "nan", "inf", "ninf")


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


@pytest.fixture(scope="module")
def cpu():
    import importlib.util

    spec = importlib.util.spec_from_file_location("imu_cpu_helpers", os.path.join(ROOT, "tests", "test_imu_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def R(cpu, tmp_path_factory):
    return cpu.build_restatement(tmp_path_factory.mktemp("imu_deskew"))


def trajectory(cpu, n_traj, motion):
    """cpu.synthetic_trajectory with stamps that whole or fractional millisecond values hit exactly: stamp = float32(ms) * 1e-3f.
    Returns (trajectory, ms)."""
    traj = cpu.synthetic_trajectory(n_traj, *MOTIONS[motion])
    ms = (traj[:, 7].astype(np.float64) * 1e3).astype(np.float32)
    ms[-1] = 100.0
    traj[:, 7] = ms * np.float32(1e-3)
    return traj, ms


@pytest.fixture(scope="module")
def cloud(cpu):
    """the big cloud with uniform stamps; 500-row groups are given their stamps per trajectory by stamps_for(). Rows 0..6 carry
    one member of each group, so that the small clouds (the first n rows) see them too."""
    pts, covs, nrm = cpu.random_cloud(N, seed=1234)
    rs = np.random.RandomState(99)
    t = rs.uniform(0, 100, N).astype(np.float32)
    pick = rs.permutation(np.arange(len(GROUPS), N))[:len(GROUPS) * 499].reshape(len(GROUPS), 499)
    rows = {name: np.r_[k, pick[k]] for k, name in enumerate(GROUPS)}
    return dict(pts=pts, covs=covs, nrm=nrm, t=t, rows=rows)


def stamps_for(cloud, ms):
    t = cloud["t"].copy()
    rows = cloud["rows"]
    t[rows["zero"]] = 0.0
    t[rows["neg"]] = -7.5
    t[rows["over"]] = 130.0
    inner = ms[:-1]  # (on the last pose alpha is 1, not 0)
    t[rows["on_stamp"]] = inner[np.arange(500) % len(inner)]
    t[rows["nan"]] = np.nan
    t[rows["inf"]] = np.inf
    t[rows["ninf"]] = -np.inf
    return t


def device_run(pts, covs, nrm, t, rows, in_place):
    """sp_deskew_imu on the arrays given (None: attribute absent); numpy results"""
    from sycl_points_amd import _lib

    L = _lib.lib()
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    P, Cv, Nr, T, Rw = dev(pts), dev(covs), dev(nrm), dev(t), dev(rows)
    if in_place:
        Po, Co, No = P, Cv, Nr
    else:
        Po, Co, No = (None if x is None else torch.full_like(x, 123.0) for x in (P, Cv, Nr))
    ptr = lambda x: None if x is None else _vp(x.data_ptr())  # noqa: E731
    rc = L.sp_deskew_imu(ptr(P), ptr(Cv), ptr(Nr), ptr(T), len(pts), ptr(Rw), len(rows), ptr(Po), ptr(Co), ptr(No),
                         _vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.sp_last_error()
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in (Po, Co, No))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n_traj", N_TRAJ)
@pytest.mark.parametrize("motion", list(MOTIONS))
def test_parity_and_exact_properties(sp, cpu, R, cloud, motion, n_traj):
    from sycl_points_amd import _lib

    pts, covs, nrm, rows = cloud["pts"], cloud["covs"], cloud["nrm"], cloud["rows"]
    traj, ms = trajectory(cpu, n_traj, motion)
    t = stamps_for(cloud, ms)
    table = cpu.lib_intervals(_lib.lib(), traj)
    ref32 = cpu.restate(R, pts, covs, nrm, t, traj)
    ref64 = cpu.restate(R, pts, covs, nrm, t, traj, f64=True)
    finite = np.isfinite(t)
    names = ("points", "covs", "normals")
    E_ref = {k: float(np.abs(a[finite].astype(np.float64) - b[finite]).max()) for k, a, b in zip(names, ref32, ref64)}
    assert E_ref["points"] > 0 and E_ref["normals"] > 0 and E_ref["covs"] > 0
    at_end = device_run(pts, covs, nrm, np.full(N, 100.0, np.float32), table, False)  # every row on the last pose
    first = None
    for attr, (with_c, with_n) in ATTRS.items():
        c_in, n_in = covs if with_c else None, nrm if with_n else None
        for in_place in (False, True):
            out = dict(zip(names, device_run(pts, c_in, n_in, t, table, in_place)))
            inp = dict(points=pts, covs=c_in, normals=n_in)
            present = [k for k in names if inp[k] is not None]
            # --- exact, bit for bit
            for k in present:
                o, i = out[k], inp[k]
                for name in ("nan", "inf", "ninf"):  # a non-finite stamp: the whole row as it was, the covariance's marker included
                    assert np.array_equal(bits(o[rows[name]]), bits(i[rows[name]])), (attr, in_place, k, name)
            for name in ("zero", "neg"):  # t <= 0: point, normal and 3x3 covariance untouched
                r = rows[name]
                assert np.array_equal(bits(out["points"][r]), bits(pts[r])), (attr, in_place, name)
                if with_n:
                    assert np.array_equal(bits(out["normals"][r][:, :3]), bits(nrm[r][:, :3]))
                if with_c:
                    o4, i4 = out["covs"][r].reshape(-1, 4, 4), covs[r].reshape(-1, 4, 4)
                    assert np.array_equal(bits(o4[:, :3, :3]), bits(i4[:, :3, :3]))
            r = rows["over"]  # past the last stamp equals on the last stamp
            assert np.array_equal(bits(out["points"][r]), bits(at_end[0][r]))
            if with_c:
                assert np.array_equal(bits(out["covs"][r]), bits(at_end[1][r]))
            if with_n:
                assert np.array_equal(bits(out["normals"][r]), bits(at_end[2][r]))
            r = rows["on_stamp"]  # exactly on a pose (the pair of equal stamps among them): alpha = 0, the restatement's bits
            for k, r32 in zip(names, ref32):
                if inp[k] is not None:
                    assert np.array_equal(bits(out[k][r]), bits(r32[r])), (attr, in_place, k)
            assert np.array_equal(bits(out["points"][:, 3]), bits(pts[:, 3]))  # w is the input's
            if with_n:
                assert not out["normals"][finite][:, 3].any()
            if with_c:
                o4 = out["covs"][finite].reshape(-1, 4, 4)
                assert not o4[:, 3, :].any() and not o4[:, :, 3].any()
            # the attribute sets do not influence each other; in place is out of place
            if first is None:
                first = out["points"]
            assert np.array_equal(bits(out["points"]), bits(first)), (attr, in_place)
            if attr == "all":
                if not in_place:
                    all_out = out
                else:
                    for k in names:
                        assert np.array_equal(bits(out[k]), bits(all_out[k])), k
            # --- the rest: against float64, with the restatement's own error as the measure
            for k, r64 in zip(names, ref64):
                if inp[k] is None:
                    continue
                E_dev = float(np.abs(out[k][finite].astype(np.float64) - r64[finite]).max())
                print(f"imu deskew parity [{motion:5s} n_traj={n_traj:4d} {attr:14s} {'in place' if in_place else 'out of place'}] "
                      f"{k:8s}: E_dev = {E_dev:.3e}  E_ref = {E_ref[k]:.3e}  m = {M_BOUND}")
                assert E_dev <= M_BOUND * E_ref[k], (motion, n_traj, attr, in_place, k, E_dev, E_ref[k])
    # the small clouds are the first rows of the big one: the same bits, whatever the grid
    for n in SMALL:
        for in_place in (False, True):
            small = device_run(pts[:n], covs[:n], nrm[:n], t[:n], table, in_place)
            for k, a in zip(names, small):
                assert np.array_equal(bits(a), bits(all_out[k][:n])), (n, in_place, k)


def test_unordered_and_equal_stamps(sp, cpu, R, cloud):
    """A table whose stamps are not ascending, with repeats: the device picks the interval the reference's bisection picks."""
    from sycl_points_amd import _lib

    n = 20000
    pts, covs, nrm = (cloud[k][:n] for k in ("pts", "covs", "nrm"))
    names = ("points", "covs", "normals")
    for n_traj in (26, 300, 5000):
        traj, ms = trajectory(cpu, n_traj, "fast")
        rs = np.random.RandomState(n_traj)
        stamps = traj[:, 7].copy()
        stamps[1:-1] = rs.permutation(stamps[1:-1])
        stamps[3:6] = stamps[3]
        traj[:, 7] = stamps
        t = stamps_for(cloud, ms)[:n]
        table = cpu.lib_intervals(_lib.lib(), traj)
        ref32 = cpu.restate(R, pts, covs, nrm, t, traj)
        ref64 = cpu.restate(R, pts, covs, nrm, t, traj, f64=True)
        out = device_run(pts, covs, nrm, t, table, False)
        finite = np.isfinite(t)
        for k, o, r32, r64 in zip(names, out, ref32, ref64):
            E_ref = float(np.abs(r32[finite].astype(np.float64) - r64[finite]).max())
            E_dev = float(np.abs(o[finite].astype(np.float64) - r64[finite]).max())
            print(f"imu deskew unordered [n_traj={n_traj:4d}] {k:8s}: E_dev = {E_dev:.3e}  E_ref = {E_ref:.3e}  m = {M_BOUND}")
            assert E_dev <= M_BOUND * E_ref, (n_traj, k, E_dev, E_ref)


def _imu_case(sp, cpu, n=20000):
    t, gyro, accel = cpu.imu_samples(200, 19.96, 0.2, seed=11)
    T_il = np.eye(4, dtype=np.float32)
    T_il[:3, :3] = cpu.rot_z(0.3)
    T_il[:3, 3] = [0.1, -0.05, 0.2]
    return dict(stamps=t, gyro=gyro, accel=accel, start=20.0013, T_il=T_il, bias=cpu.BIAS_LIN, Rwb=cpu.rot_z(-0.4),
                v=np.array([3.0, -1.0, 0.2], np.float32))


def test_python_mirror(sp, cpu, cloud):
    from sycl_points_amd import _lib

    n = 20000
    pts, covs, nrm, t = (cloud[k][:n] for k in ("pts", "covs", "nrm", "t"))
    c = _imu_case(sp, cpu)
    for gyro_only in (False, True):
        pc = sp.PointCloudShared.from_numpy(pts, covs=covs, normals=nrm, timestamp_offsets=t)
        pc.start_time_ms, pc.end_time_ms = 20001.3, 20101.3
        prm = sp.IMUPreintegrationParams()
        out, status = sp.deskew_point_cloud_imu(pc, c["stamps"], c["gyro"], c["accel"], c["start"], c["T_il"], c["bias"], prm, c["Rwb"],
                                                c["v"], gyro_only=gyro_only)
        assert status == sp.IMUDeskewStatus.success
        rc, st, traj = cpu.c_trajectory(_lib.lib(), c["stamps"], c["gyro"], c["accel"], c["start"], (20101.3 - 20001.3) * 1e-3,
                                        gyro_only=gyro_only, bias=c["bias"], T_il=c["T_il"], Rwb=c["Rwb"], v=c["v"])
        assert (rc, st) == (0, 0)
        ref = device_run(pts, covs, nrm, t, cpu.lib_intervals(_lib.lib(), traj), False)
        assert out is not pc and out.points.data_ptr() != pc.points.data_ptr()
        for a, b in zip((out.points, out.covs, out.normals), ref):
            assert np.array_equal(bits(a.cpu().numpy()), bits(b))
        assert out.timestamp_offsets is pc.timestamp_offsets and (out.start_time_ms, out.end_time_ms) == (20001.3, 20101.3)
        assert np.array_equal(pc.points.cpu().numpy(), pts)  # the input is left alone
        assert not np.array_equal(out.points.cpu().numpy()[:, :3], pts[:, :3])


# ------------------------------------------------------------------------------------------------ the reference's physical cases
kEps = 5e-3  # cpp/tests/test_imu_deskew.cpp:19 (5 mm)


def _rz64(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])


def _cloud(sp, points, offsets_ms, start_sec, normals=None, covs=None):
    p = np.ones((len(points), 4), np.float32)
    p[:, :3] = points
    pc = sp.PointCloudShared.from_numpy(p, timestamp_offsets=np.array(offsets_ms, np.float32), normals=normals, covs=covs)
    pc.start_time_ms, pc.end_time_ms = start_sec * 1e3, (start_sec + 0.1) * 1e3
    return pc


def test_reference_physical_cases(sp, cpu):
    """cpp/tests/test_imu_deskew.cpp:48-220, 356-478 through api, within the reference's 5 mm / 5e-3"""
    no_g = sp.IMUPreintegrationParams(gravity=(0.0, 0.0, 0.0))
    I4 = np.eye(4, dtype=np.float32)
    # PureRotationDeskew and its gyro_only twin
    start, omega = 1.0, np.float32(np.pi) / np.float32(2.0)
    world = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0.5], [-1, 0.5, 0], [0.5, -0.5, 1]], np.float64)
    off = [0.0, 25.0, 50.0, 75.0, 100.0]
    sensor = np.array([_rz64(float(omega) * o * 1e-3).T @ w for o, w in zip(off, world)])
    buf = cpu.make_imu_buffer(start - 0.02, 0.14, 24, (0, 0, omega), (0, 0, 0))
    for gyro_only in (False, True):
        out, st = sp.deskew_point_cloud_imu(_cloud(sp, sensor, off, start), *buf, start, I4, None, no_g, gyro_only=gyro_only)
        assert st == sp.IMUDeskewStatus.success and out.size() == 5
        assert np.linalg.norm(out.points.cpu().numpy()[:, :3] - world, axis=1).max() <= kEps
    # PureTranslationDeskew: 1 m/s^2 along x from rest
    start = 2.0
    world = np.array([[2, 0, 0], [0, 2, 0], [1, 1, 1]], np.float64)
    off = [0.0, 50.0, 100.0]
    sensor = np.array([w - [0.5 * (o * 1e-3) ** 2, 0, 0] for o, w in zip(off, world)])
    buf = cpu.make_imu_buffer(start - 0.02, 0.14, 24, (0, 0, 0), (1.0, 0, 0))
    out, st = sp.deskew_point_cloud_imu(_cloud(sp, sensor, off, start), *buf, start, I4, None, no_g)
    assert st == sp.IMUDeskewStatus.success
    assert np.linalg.norm(out.points.cpu().numpy()[:, :3] - world, axis=1).max() <= kEps
    # GyroOnlyIgnoresAccelerationAndInitialVelocity
    start = 3.0
    inp = np.array([[1, 2, 3], [-2, 0.5, 1], [0.25, -0.75, 4]], np.float64)
    buf = cpu.make_imu_buffer(start - 0.02, 0.14, 24, (0, 0, 0), (3.0, -2.0, 11.0))
    out, st = sp.deskew_point_cloud_imu(_cloud(sp, inp, off, start), *buf, start, I4, None, sp.IMUPreintegrationParams(),
                                        v_world=(5.0, -4.0, 2.0), gyro_only=True)
    assert st == sp.IMUDeskewStatus.success
    assert np.linalg.norm(out.points.cpu().numpy()[:, :3] - inp, axis=1).max() <= kEps
    # MatchesConstantVelocityApproximately
    start, omega = 0.0, np.float32(np.pi) / np.float32(4.0)
    wp = np.array([1.0, 0.5, 0.0])
    sensor = np.array([_rz64(float(omega) * o * 1e-3).T @ wp for o in off])
    buf = cpu.make_imu_buffer(start - 0.02, 0.14, 24, (0, 0, omega), (0, 0, 0))
    pc = _cloud(sp, sensor, off, start)
    out, st = sp.deskew_point_cloud_imu(pc, *buf, start, I4, None, no_g)
    end_pose = np.eye(4, dtype=np.float32)
    end_pose[:3, :3] = _rz64(float(omega) * 0.1)
    cv = sp.deskew_point_cloud_constant_velocity(pc, I4, end_pose)
    assert st == sp.IMUDeskewStatus.success and cv is not None
    assert np.linalg.norm(out.points.cpu().numpy()[:, :3] - wp, axis=1).max() <= kEps
    assert np.linalg.norm(cv.points.cpu().numpy()[:, :3] - wp, axis=1).max() <= kEps
    # NormalsAndCovariancesRotated
    omega = np.float32(np.pi) / np.float32(2.0)
    wp, wn, wc = np.array([1.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]), np.diag([0.01, 0.02, 0.03])
    P, Nn, Cc = [], np.zeros((3, 4), np.float32), np.zeros((3, 4, 4), np.float32)
    for i, o in enumerate(off):
        Rt = _rz64(float(omega) * o * 1e-3).T
        P.append(Rt @ wp)
        Nn[i, :3] = Rt @ wn
        Cc[i, :3, :3] = Rt @ wc @ Rt.T
    buf = cpu.make_imu_buffer(-0.02, 0.14, 24, (0, 0, omega), (0, 0, 0))
    out, st = sp.deskew_point_cloud_imu(_cloud(sp, np.array(P), off, 0.0, normals=Nn, covs=Cc.transpose(0, 2, 1).reshape(3, 16)), *buf,
                                        0.0, I4, None, no_g)
    assert st == sp.IMUDeskewStatus.success
    assert np.linalg.norm(out.points.cpu().numpy()[:, :3] - wp, axis=1).max() <= kEps
    assert np.linalg.norm(out.normals.cpu().numpy()[:, :3] - wn, axis=1).max() <= kEps
    oc = out.covs.cpu().numpy().reshape(3, 4, 4).transpose(0, 2, 1)[:, :3, :3]
    assert max(np.linalg.norm(oc[i] - wc) for i in range(3)) <= kEps


def test_cpp_facade(sp):
    """tests/cpp/test_imu.cpp, built with tests/cpp/Makefile's flags and libraries (the Makefile is not changed): the reference's
    IMUPreintegration and IMUDeskewTest cases through the C++ facade, the in-place deviation, the mirrored metadata."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(cpp, "test_imu")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    lib = os.path.join(ROOT, "sycl_points_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++20", f"-I{ROOT}/include", f"-I{rocm}/include", "-D__HIP_PLATFORM_AMD__", "-Wall",
                           "-Wno-unused-value", "-Wno-unused-result", os.path.join(cpp, "test_imu.cpp"), "-o", exe,
                           f"-L{lib}", "-lsycl_points_amd", f"-Wl,-rpath,{lib}", f"-L{rocm}/lib", "-lamdhip64",
                           f"-Wl,-rpath,{rocm}/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failed" in r.stdout
