"""Constant-velocity deskew without a device: the C ABI's exports and argument checks (sp_deskew_constant_velocity returns
SP_ERR_INVALID_ARGUMENT before any HIP call), sp_relative_twist_host against float64, and the CPU restatement of the reference
kernel (tests/cpp/deskew_restate.cpp; deskew/relative_pose_deskew.hpp:120-172) on the reference's known answer and on the
exact properties the GPU suite (tests/test_gpu_deskew.py) then holds the device to bit for bit.

(Bit-identity at t = 0 is stated for coordinates that are not -0.0: the fma chain of multiply<4,4> starts from +0, so a -0.0
coordinate comes out +0.0, in the reference as here.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libdeskew_restate.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "deskew_restate.cpp"), "-o", so])
    R = C.CDLL(so)
    for name in ("deskew_restate", "deskew_f64"):
        fn = getattr(R, name)
        fn.restype = None
        fn.argtypes = [_vp, _vp, _vp, _vp, C.c_uint64, _vp, C.c_float, _vp, _vp, _vp]
    R.relative_twist_restate.restype = None
    R.relative_twist_restate.argtypes = [_vp, _vp, _vp]
    return R


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return build_restatement(tmp_path_factory.mktemp("deskew"))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def restate(R, pts, covs, nrm, t_ms, twist, duration, f64=False, in_place=False):
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
    tw = np.ascontiguousarray(twist, np.float32)
    (R.deskew_f64 if f64 else R.deskew_restate)(_ptr(pts), _ptr(covs), _ptr(nrm), _ptr(t_ms), len(pts), _ptr(tw), duration,
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


def twist_of(angle, dist, seed=5):
    rs = np.random.RandomState(seed)
    ax, d = rs.normal(size=3), rs.normal(size=3)
    return np.r_[ax / np.linalg.norm(ax) * angle, d / np.linalg.norm(d) * dist].astype(np.float32)


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbols_exported_and_listed(L):
    from sycl_points_amd import _lib

    for name in ("sp_deskew_constant_velocity", "sp_relative_twist_host"):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
    with open(os.path.join(ROOT, "include", "sycl_points_amd.h")) as f:
        hdr = f.read()
    assert "sp_deskew_constant_velocity(" in hdr and "sp_relative_twist_host(" in hdr
    assert L.sp_abi_version() == 7


def test_invalid_arguments_need_no_device(L):
    from sycl_points_amd import _lib

    a = np.zeros((8, 16), np.float32)
    tw = np.zeros(6, np.float32)
    P = _ptr(a)
    TW = _ptr(tw)
    ok = dict(points=P, covs=None, normals=None, ts=P, n=8, twist=TW, dur=0.1, po=P, co=None, no=None)
    cases = [dict(points=None), dict(ts=None), dict(po=None), dict(twist=None),
             dict(covs=P), dict(co=P), dict(normals=P), dict(no=P),             # an attribute without its other half
             dict(dur=0.0), dict(dur=-0.1), dict(dur=float("inf")), dict(dur=float("nan")),
             dict(n=1 << 32), dict(n=(1 << 32) + 5)]
    for c in cases:
        k = {**ok, **c}
        rc = L.sp_deskew_constant_velocity(k["points"], k["covs"], k["normals"], k["ts"], k["n"], k["twist"], k["dur"], k["po"],
                                           k["co"], k["no"], None)
        assert rc == _lib.SP_ERR_INVALID_ARGUMENT, c
        assert b"sp_deskew_constant_velocity" in L.sp_last_error()
    # n == 0: SP_OK, nothing enqueued (no device is needed for it)
    assert L.sp_deskew_constant_velocity(P, None, None, P, 0, TW, 0.1, P, None, None, None) == 0


def _se3_log_f64(T):
    """rotation-first twist of a rigid transform in float64 (eigen_utils.hpp:991-1034's formula)"""
    Rm, t = T[:3, :3], T[:3, 3]
    v = 0.5 * np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])
    s, c = np.linalg.norm(v), 0.5 * (np.trace(Rm) - 1.0)
    theta = np.arctan2(s, c)
    w = v * (theta / s) if s > 1e-12 else v
    O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    Vi = np.eye(3) - 0.5 * O
    if theta > 1e-6:
        Vi = Vi + (1.0 - theta * np.cos(0.5 * theta) / (2.0 * np.sin(0.5 * theta))) / theta ** 2 * (O @ O)
    else:
        Vi = Vi + (O @ O) / 12.0
    return np.r_[w, Vi @ t]


def test_relative_twist_against_float64(L):
    from oracle.pyoracle import Oracle

    orc = Oracle()
    rng = np.random.default_rng(3)
    out = np.zeros(6, np.float32)
    # (poses a scan apart: relative rotations of up to about a radian. The logarithm's conditioning grows as 1 / (pi - angle), so
    # near half a turn float32 cannot hold a bound of a few ulp against float64 whatever the code does.)
    for mag in (1e-8, 1e-3, 0.05, 0.3):
        for _ in range(6):
            Tp = orc.se3_exp(rng.normal(size=6).astype(np.float32) * np.float32(mag))
            Tc = orc.se3_exp(rng.normal(size=6).astype(np.float32) * np.float32(mag))
            L.sp_relative_twist_host(_ptr(np.ascontiguousarray(Tp.T)), _ptr(np.ascontiguousarray(Tc.T)), _ptr(out))
            ref = _se3_log_f64(np.linalg.inv(Tp.astype(np.float64)) @ Tc.astype(np.float64))
            assert np.abs(out - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max()), (mag, out, ref)  # test_host_terms.py's bound
    # identical poses: the zero twist exactly (R^T R is formed symmetric and R^T t cancels term by term)
    T = np.ascontiguousarray(orc.se3_exp(np.array([0.3, -0.2, 0.5, 1.0, 2.0, -3.0], np.float32)).T)
    for pose in (np.ascontiguousarray(np.eye(4, dtype=np.float32)), T):
        out[:] = 1.0
        L.sp_relative_twist_host(_ptr(pose), _ptr(pose), _ptr(out))
        assert not out.any(), out


def test_resource_report_has_no_scratch(L):
    path = os.path.join(ROOT, "sycl_points_amd", "lib", "deskew.resources.txt")
    with open(path) as f:
        rows = [r for r in f.read().splitlines() if "deskew_kernel" in r]
    assert len(rows) == 4, rows  # points | + covs | + normals | + both
    for r in rows:
        assert re.search(r"VGPRs Spill: 0\b", r) and re.search(r"ScratchSize \[bytes/lane\]: 0\b", r), r


# ------------------------------------------------------------------------------------------------ the restatement
def test_reference_known_answer(R, L):
    """cpp/tests/test_relative_pose_deskew.cpp:13-76: identity -> (1 m along x, 90 deg about z) over the scan; a world point
    (1, 1, 0), normal z, covariance diag(0.01, 0.02, 0.03) observed from the moving sensor at 0, 500 and 1000 ms; every deskewed
    point and normal within 1e-5 (norm) and every covariance within 1e-6 (Frobenius) of the world values."""
    prev = np.eye(4)
    ang = np.pi / 2
    cur = np.eye(4)
    cur[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    cur[:3, 3] = [1.0, 0.0, 0.0]
    prev32, cur32 = prev.astype(np.float32), cur.astype(np.float32)
    twist = np.zeros(6, np.float32)
    L.sp_relative_twist_host(_ptr(np.ascontiguousarray(prev32.T)), _ptr(np.ascontiguousarray(cur32.T)), _ptr(twist))
    twist_r = np.zeros(6, np.float32)
    R.relative_twist_restate(_ptr(np.ascontiguousarray(prev32.T)), _ptr(np.ascontiguousarray(cur32.T)), _ptr(twist_r))
    assert np.abs(twist - twist_r).max() <= 2e-6
    tw64 = _se3_log_f64(np.linalg.inv(prev) @ cur)
    Pw, Nw, Cw = np.array([1.0, 1.0, 0.0, 1.0]), np.array([0.0, 0.0, 1.0]), np.diag([0.01, 0.02, 0.03])
    t_ms = np.array([0.0, 500.0, 1000.0], np.float32)
    pts, nrm, covs = np.zeros((3, 4), np.float32), np.zeros((3, 4), np.float32), np.zeros((3, 4, 4), np.float32)

    def se3_exp64(a):
        w, v = a[:3], a[3:]
        th = np.linalg.norm(w)
        O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        T = np.eye(4)
        if th < 1e-12:
            T[:3, 3] = v
            return T
        T[:3, :3] = np.eye(3) + np.sin(th) / th * O + (1 - np.cos(th)) / th ** 2 * (O @ O)
        T[:3, 3] = (np.eye(3) + (1 - np.cos(th)) / th ** 2 * O + (th - np.sin(th)) / th ** 3 * (O @ O)) @ v
        return T

    for i, t in enumerate(t_ms):
        pose_t = prev @ se3_exp64(tw64 * (t / 1000.0))  # the sensor at the sampling time (constant body velocity)
        inv = np.linalg.inv(pose_t)
        pts[i] = inv @ Pw
        nrm[i, :3] = inv[:3, :3] @ Nw
        covs[i, :3, :3] = inv[:3, :3] @ Cw @ inv[:3, :3].T
    po, co, no = restate(R, pts, covs.transpose(0, 2, 1).reshape(3, 16), nrm, t_ms, twist, 1.0)
    for i in range(3):
        assert np.linalg.norm(po[i, :3] - Pw[:3]) <= 1e-5 and po[i, 3] == 1.0, (i, po[i])
        assert np.linalg.norm(no[i, :3] - Nw) <= 1e-5 and no[i, 3] == 0.0
        Cgot = co[i].reshape(4, 4).T
        assert np.linalg.norm(Cgot[:3, :3] - Cw) <= 1e-6
        assert not Cgot[3].any() and not Cgot[:, 3].any()
    assert np.linalg.norm(pts[1, :3] - Pw[:3]) > 0.3  # (the sample at 500 ms was observed somewhere else)


def test_exact_properties(R):
    n = 4000
    pts, covs, nrm = random_cloud(n, seed=7)
    rs = np.random.RandomState(1)
    pts[:, 3] = rs.choice([1.0, 0.0, 2.5], n).astype(np.float32)  # w is carried, whatever it is
    duration = 0.1
    for angle, dist in ((0.05, 1.5), (2e-3, 0.2), (1e-7, 0.0)):
        tw = twist_of(angle, dist)
        # t = 0: point, normal and the 3x3 covariance bit-identical; normal w and the covariance's fourth row / column are 0
        t0 = np.zeros(n, np.float32)
        po, co, no = restate(R, pts, covs, nrm, t0, tw, duration)
        assert np.array_equal(po.view(np.uint32), pts.view(np.uint32))
        assert np.array_equal(no[:, :3].view(np.uint32), nrm[:, :3].view(np.uint32)) and not no[:, 3].any()
        c4, i4 = co.reshape(n, 4, 4), covs.reshape(n, 4, 4)
        assert np.array_equal(c4[:, :3, :3].view(np.uint32), i4[:, :3, :3].view(np.uint32))
        assert not c4[:, 3, :].any() and not c4[:, :, 3].any()
        # t < 0 equals t = 0; t > duration equals t = duration
        neg = restate(R, pts, covs, nrm, np.full(n, -3.0, np.float32), tw, duration)
        full = restate(R, pts, covs, nrm, np.full(n, 100.0, np.float32), tw, duration)
        over = restate(R, pts, covs, nrm, np.full(n, 250.0, np.float32), tw, duration)
        for a, b in zip(neg, (po, co, no)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        for a, b in zip(over, full):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # a non-finite time stamp: every row bit-identical, the covariance's fourth row and column included
        for bad in (np.nan, np.inf, -np.inf):
            cp = restate(R, pts, covs, nrm, np.full(n, bad, np.float32), tw, duration)
            for a, b in zip(cp, (pts, covs, nrm)):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # anywhere in between: w is the input's, normal w and the covariance's fourth row / column are exactly 0
        tm = rs.uniform(0, 100, n).astype(np.float32)
        pm, cm, nm = restate(R, pts, covs, nrm, tm, tw, duration)
        assert np.array_equal(pm[:, 3].view(np.uint32), pts[:, 3].view(np.uint32))
        assert not nm[:, 3].any()
        cm4 = cm.reshape(n, 4, 4)
        assert not cm4[:, 3, :].any() and not cm4[:, :, 3].any()
        if angle > 1e-3:
            assert not np.array_equal(pm[:, :3], pts[:, :3])
        # the attribute sets do not influence each other, and in place is out of place
        assert np.array_equal(restate(R, pts, None, None, tm, tw, duration)[0].view(np.uint32), pm.view(np.uint32))
        ip = restate(R, pts, covs, nrm, tm, tw, duration, in_place=True)
        for a, b in zip(ip, (pm, cm, nm)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_restatement_against_float64(R):
    """The float32 restatement stays within float32 rounding of the float64 evaluation of the same formula (the yardstick the GPU
    suite measures the device with): positions of up to 87 m, so 1e-4 absolute is ~15 ulp of the largest coordinate."""
    n = 20000
    pts, covs, nrm = random_cloud(n, seed=11)
    tm = np.random.RandomState(2).uniform(0, 100, n).astype(np.float32)
    for angle, dist in ((0.05, 1.5), (2e-3, 0.2), (1e-7, 0.0)):
        tw = twist_of(angle, dist)
        a = restate(R, pts, covs, nrm, tm, tw, 0.1)
        b = restate(R, pts, covs, nrm, tm, tw, 0.1, f64=True)
        assert np.abs(a[0] - b[0]).max() <= 1e-4
        assert np.abs(a[2] - b[2]).max() <= 1e-6
        assert np.abs(a[1] - b[1]).max() <= 1e-6 * np.abs(b[1]).max()
