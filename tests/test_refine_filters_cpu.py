"""The scan filters that follow kNN and covariances, without a device: the C ABI's exports and argument checks
(sp_angle_incidence_flags, sp_intensity_correct and sp_intensity_gaussian return their errors before any HIP call, with the
reference's texts), and the CPU restatement of the four per-point formulas (tests/cpp/refine_restate.cpp) on the reference's
known answers and on the exact properties the GPU suite (tests/test_gpu_refine_filters.py) then holds the device to.

The helpers here (the restatement's wrappers, the planes cloud and its planted rows) are the GPU suite's too."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
_f = C.c_float
_u64 = C.c_uint64


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "librefine_restate.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "refine_restate.cpp"), "-o", so])
    R = C.CDLL(so)
    for name in ("angle_flags_restate", "angle_flags_f64"):
        getattr(R, name).restype = None
        getattr(R, name).argtypes = [_vp, _vp, _u64, _f, _f, _vp]
    for name in ("intensity_correct_restate", "intensity_correct_f64"):
        getattr(R, name).restype = None
        getattr(R, name).argtypes = [_vp, _vp, _vp, _u64, _f, _f, _f, _f, _f, _f, _vp]
    for name in ("intensity_gaussian_restate", "intensity_gaussian_f64"):
        getattr(R, name).restype = None
        getattr(R, name).argtypes = [_vp, _vp, _vp, _u64, _u64, _u64, _f, _f, _f, _f, _vp, _vp, _vp]
    return R


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return build_restatement(tmp_path_factory.mktemp("refine"))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def angle_flags(R, pts, nrm, min_angle, max_angle, f64=False):
    pts, nrm = _f32(pts), _f32(nrm)
    flags = np.full(len(pts), 7, np.uint8)
    (R.angle_flags_f64 if f64 else R.angle_flags_restate)(_ptr(pts), _ptr(nrm), len(pts), min_angle, max_angle, _ptr(flags))
    return flags


def correct(R, pts, nrm, inten, exponent=2.0, scale=1.0, lo=0.0, hi=1000.0, ref=1.0, angle_exponent=0.0, f64=False):
    pts, nrm, inten = _f32(pts), _f32(nrm), _f32(inten)
    out = np.empty(len(pts), np.float64 if f64 else np.float32)
    (R.intensity_correct_f64 if f64 else R.intensity_correct_restate)(_ptr(pts), _ptr(nrm), _ptr(inten), len(pts), exponent, scale, lo,
                                                                     hi, ref, angle_exponent, _ptr(out))
    return out


def gaussian(R, pts, inten, knn, s_az, s_el, s_r=0.05, mean_min=0.0, k_limit=0, f64=False, exponents=False):
    """the smoothed (mean_min <= 0) or normalised intensities; with exponents=True also each row's smallest and largest exponent"""
    pts, inten = _f32(pts), _f32(inten)
    knn = np.ascontiguousarray(knn, np.int32)
    n, k = knn.shape
    k_use = k_limit if 0 < k_limit < k else k
    out = np.empty(n, np.float64 if f64 else np.float32)
    emin, emax = np.empty(n, np.float64), np.empty(n, np.float64)
    (R.intensity_gaussian_f64 if f64 else R.intensity_gaussian_restate)(_ptr(pts), _ptr(inten), _ptr(knn), n, k, k_use, s_az, s_el, s_r,
                                                                       mean_min, _ptr(out), _ptr(emin), _ptr(emax))
    return (out, emin, emax) if exponents else out


def knn_numpy(pts, k):
    """exact k nearest neighbours (self first) of a small cloud, -1 padding when it has fewer than k points"""
    n = len(pts)
    p = pts[:, :3].astype(np.float64)
    out = np.full((n, k), -1, np.int32)
    for a in range(0, n, 512):
        d = ((p[a:a + 512, None, :] - p[None, :, :]) ** 2).sum(-1)
        order = np.argsort(d, axis=1, kind="stable")[:, :k]
        out[a:a + 512, :order.shape[1]] = order
    return out


def planes_cloud(n, seed=2024):
    """n points on three noisy planes around the origin (z = -1.5 seen from above, x = 3 and y = -2.5 seen obliquely), thickness
    0.01, about 0.1 apart; w = 1; intensities U[0, 255); time stamps U[0, 100)"""
    rs = np.random.RandomState(seed)
    side = np.sqrt(n / 3.0) * 0.1
    uv = rs.uniform(-0.5 * side, 0.5 * side, (n, 2))
    noise = rs.normal(0.0, 0.01, n)
    which = np.arange(n) % 3
    pts = np.ones((n, 4), np.float32)
    for w, (axis, offset) in enumerate(((2, -1.5), (0, 3.0), (1, -2.5))):
        m = which == w
        others = [a for a in range(3) if a != axis]
        pts[m, others[0]] = uv[m, 0]
        pts[m, others[1]] = uv[m, 1]
        pts[m, axis] = offset + noise[m]
    inten = rs.uniform(0.0, 255.0, n).astype(np.float32)
    stamps = rs.uniform(0.0, 100.0, n).astype(np.float32)
    return pts, inten, stamps


# rows of the planes cloud that are overwritten AFTER kNN, covariances and normals were computed on the clean cloud
PLANTED = dict(nan=11, inf=12, zero_normal=13, origin=14, zenith=(15, 16, 17), far=18, out_of_range=(19, 20, 21, 22))


def plant_rows(pts, nrm, covs, knn):
    """The special rows (copies are returned): a NaN point, an Inf point, a zero normal (and covariance), a point at the origin,
    three points on / next to the z axis that list each other and then padding, a row whose ten listed neighbours are the ten
    points farthest from it, and four rows with indices outside [0, n) among their neighbours. Returns the arrays and the boolean
    mask of the rows that are none of these and list none of them (the `regular` rows)."""
    pts, nrm, covs, knn = pts.copy(), nrm.copy(), covs.copy(), knn.copy()
    n, k = knn.shape
    P = PLANTED
    pts[P["nan"], 0] = np.nan
    pts[P["inf"], 1] = np.inf
    nrm[P["zero_normal"]] = 0.0
    covs[P["zero_normal"]] = 0.0
    pts[P["origin"]] = (0.0, 0.0, 0.0, 1.0)
    z = P["zenith"]
    pts[z[0]], pts[z[1]], pts[z[2]] = (0.0, 0.0, 5.0, 1.0), (0.0, 0.0, 5.05, 1.0), (0.05, 0.0, 5.0, 1.0)
    for a in z:
        knn[a] = -1
        knn[a, :min(3, k)] = ([a] + [b for b in z if b != a])[:min(3, k)]
    if n > 100:
        d = np.linalg.norm(pts[:, :3].astype(np.float64) - pts[P["far"], :3], axis=1)
        d[~np.isfinite(d)] = -1.0
        knn[P["far"]] = np.argsort(d)[-k:]
    bad = (n, n + 5, 2 ** 31 - 1, -7)
    for a, b in zip(P["out_of_range"], bad):
        knn[a, (1 + a) % k] = b
        knn[a, (4 + a) % k] = -1
    planted = np.zeros(n, bool)
    idx = [P["nan"], P["inf"], P["zero_normal"], P["origin"], *P["zenith"], P["far"], *P["out_of_range"]]
    planted[idx] = True
    listed = np.isin(knn, idx).any(axis=1)
    return pts, nrm, covs, knn, ~planted & ~listed


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbols_exported_and_listed(L):
    from sycl_points_amd import _lib

    with open(os.path.join(ROOT, "include", "sycl_points_amd.h")) as f:
        hdr = f.read()
    for name in ("sp_angle_incidence_flags", "sp_intensity_correct", "sp_intensity_gaussian"):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
        assert name + "(" in hdr
    assert hasattr(L, "sp_compact_by_flags_multi")  # the fourth symbol of the stage: the compaction the angle filter hands over to
    assert L.sp_abi_version() == 7
    for name in ("intensity_correction", "intensity_gaussian", "intensity_local_mean_norm"):
        assert os.path.exists(os.path.join(ROOT, "include", "sycl_points", "algorithms", "filter", name + ".hpp"))


def test_python_mirror_is_there():
    import sycl_points_amd.api as api

    for name in ("angle_incidence_filter", "correct_intensity", "smooth_intensity", "normalize_intensity_local_mean"):
        assert callable(getattr(api, name))


def test_invalid_arguments_need_no_device(L):
    from sycl_points_amd import _lib

    a = np.zeros((8, 16), np.float32)
    b = np.zeros((8, 16), np.float32)
    P, Q = _ptr(a), _ptr(b)
    RT, IA = _lib.SP_ERR_RUNTIME, _lib.SP_ERR_INVALID_ARGUMENT
    half_pi = float(np.float32(np.pi) * np.float32(0.5))

    def angle(points=P, normals=P, covs=None, n=8, lo=0.2, hi=1.2, flags=Q):
        return L.sp_angle_incidence_flags(points, normals, covs, n, lo, hi, flags, None)

    for kw, code, text in [
            (dict(normals=None), RT, b"[PreprocessFilter::angle_incidence_filter] Normal vector or covariance matrices must be pre-computed."),
            (dict(lo=-0.1), IA, b"[PreprocessFilter::angle_incidence_filter] Invalid angle range"),
            (dict(hi=float(np.nextafter(np.float32(half_pi), np.float32(4)))), IA, b"[PreprocessFilter::angle_incidence_filter] Invalid angle range"),
            (dict(lo=0.7, hi=0.7), IA, b"[PreprocessFilter::angle_incidence_filter] Invalid angle range"),
            (dict(lo=0.9, hi=0.7), IA, b"[PreprocessFilter::angle_incidence_filter] Invalid angle range"),
            (dict(normals=None, lo=-1.0), RT, b"must be pre-computed."),  # the reference's order: the attributes first
            (dict(points=None), IA, b"sp_angle_incidence_flags"), (dict(flags=None), IA, b"sp_angle_incidence_flags"),
            (dict(n=1 << 32), IA, b"sp_angle_incidence_flags")]:
        assert angle(**kw) == code, kw
        assert L.sp_last_error().endswith(text) or text in L.sp_last_error(), (kw, L.sp_last_error())
    assert angle(n=0, normals=None, lo=-1.0) == 0  # an empty cloud: before any check

    def corr(points=P, normals=None, covs=None, inten=Q, n=8, e=2.0, ref=1.0, ae=0.0):
        return L.sp_intensity_correct(points, normals, covs, inten, n, e, 1.0, 0.0, 1000.0, ref, ae, None)

    for kw, code, text in [(dict(e=-0.5), RT, b"[correct_intensity] exponent must be non-negative"),
                           (dict(ref=0.0), RT, b"[correct_intensity] ref_distance must be positive"),
                           (dict(ref=-1.0), RT, b"[correct_intensity] ref_distance must be positive"),
                           (dict(inten=None), RT, b"[correct_intensity] Intensity field not found"),
                           (dict(e=-1.0, ref=0.0, inten=None), RT, b"[correct_intensity] exponent must be non-negative"),
                           (dict(points=None), IA, b"sp_intensity_correct"), (dict(n=1 << 32), IA, b"sp_intensity_correct")]:
        assert corr(**kw) == code, kw
        assert L.sp_last_error() == text or text in L.sp_last_error(), (kw, L.sp_last_error())
    assert corr(n=0, e=-1.0) == 0

    idx = np.zeros((8, 10), np.int32)
    K = _ptr(idx)

    def gauss(points=P, i_in=P, knn=K, n=8, ks=10, ku=10, s=(0.1, 0.1, 0.05), mean_min=0.0, out=Q):
        return L.sp_intensity_gaussian(points, i_in, knn, n, ks, ku, s[0], s[1], s[2], mean_min, out, None)

    for mean_min, who in ((0.0, b"[intensity_gaussian::smooth_intensity]"), (1e-3, b"[intensity_local_mean_norm::normalize]")):
        for kw, code, text in [(dict(i_in=None), RT, who + b" Intensity field not found"),
                               (dict(ks=0, ku=0), RT, who + b" neighbors.k must be >= 1"),
                               (dict(s=(0.0, 0.1, 0.1)), RT, who + b" All sigma values must be positive"),
                               (dict(s=(0.1, -1.0, 0.1)), RT, who + b" All sigma values must be positive"),
                               (dict(s=(0.1, 0.1, 0.0)), RT, who + b" All sigma values must be positive"),
                               (dict(out=P), IA, b"intensities_out must not be intensities_in"),
                               (dict(ku=0), IA, b"sp_intensity_gaussian"), (dict(ku=11), IA, b"sp_intensity_gaussian"),
                               (dict(points=None), IA, b"sp_intensity_gaussian"), (dict(knn=None), IA, b"sp_intensity_gaussian"),
                               (dict(out=None), IA, b"sp_intensity_gaussian"), (dict(n=1 << 31), IA, b"sp_intensity_gaussian")]:
            assert gauss(mean_min=mean_min, **kw) == code, kw
            assert L.sp_last_error() == text or text in L.sp_last_error(), (kw, L.sp_last_error())
        assert gauss(mean_min=mean_min, n=0, ks=0, out=P) == 0


def test_resource_report_has_no_scratch(L):
    path = os.path.join(ROOT, "sycl_points_amd", "lib", "scan_refine.resources.txt")
    with open(path) as f:
        rows = f.read().splitlines()
    for kernel, count in (("angle_flags_kernel", 2), ("intensity_correct_kernel", 3), ("intensity_gaussian_kernel", 4)):
        mine = [r for r in rows if kernel in r]
        assert len(mine) == count, (kernel, mine)
        for r in mine:
            assert re.search(r"VGPRs Spill: 0\b", r) and re.search(r"ScratchSize \[bytes/lane\]: 0\b", r), r


# ------------------------------------------------------------------------------------------------ the reference's known answers
ARC5 = np.array([[3, -0.2, 0, 1], [3, -0.1, 0, 1], [3, 0, 0, 1], [3, 0.1, 0, 1], [3, 0.2, 0, 1]], np.float32)
ARC3 = ARC5[1:4]


def test_angle_filter_known_answer(R):
    """cpp/tests/test_preprocess_filter.cpp:668-693: 0, 45 and 90 degrees against [0.2, 1.2]: only (1, 1, 0) survives"""
    pts = np.array([[1, 0, 0, 1], [1, 1, 0, 1], [0, 0, 1, 1]], np.float32)
    nrm = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0]], np.float32)
    for f64 in (False, True):
        assert angle_flags(R, pts, nrm, 0.2, 1.2, f64=f64).tolist() == [0, 1, 0]


def test_intensity_correction_known_answers(R):
    """cpp/tests/test_intensity_correction.cpp: distance compensation at exponents 2 and 1 with a clamp at 10, the reference
    distance, and the angle factor (1 at 0 degrees, 2 at 60 degrees with angle_exponent 1)"""
    pts = np.array([[1, 0, 0, 1], [0, 3, 4, 1], [1, 2, 2, 1]], np.float32)
    inten = np.array([10, 2, 1], np.float32)
    assert np.abs(correct(R, pts, None, inten, 2.0, 1.0, 0.0, 10.0) - [10.0, 10.0, 9.0]).max() <= 1e-5
    assert np.abs(correct(R, pts, None, inten, 1.0, 1.0, 0.0, 10.0) - [10.0, 10.0, 3.0]).max() <= 1e-5
    got = correct(R, pts[[1, 0]], None, np.array([10, 10], np.float32), 2.0, 1.0, 0.0, 1000.0, ref=5.0)
    assert np.abs(got - [10.0, 0.4]).max() <= 1e-4
    p2 = np.array([[0, 0, 5, 1], [0, 0, 5, 1]], np.float32)
    third = np.float32(np.pi) / np.float32(3)
    n2 = np.array([[0, 0, 1, 0], [0, np.sin(third), np.cos(third), 0]], np.float32)
    got = correct(R, p2, n2, np.ones(2, np.float32), 2.0, 1.0, 0.0, 1000.0, ref=5.0, angle_exponent=1.0)
    assert np.abs(got - [1.0, 2.0]).max() <= 1e-4


def test_gaussian_known_answers(R):
    """cpp/tests/test_intensity_gaussian.cpp:23-148"""
    # a spike in the middle of an arc spreads out
    out = gaussian(R, ARC5, [0, 0, 1, 0, 0], knn_numpy(ARC5, 5), 0.3, 0.3, 0.3)
    assert out[2] < 1.0 and out[1] > 0.0 and out[3] > 0.0
    # a wide azimuth sigma blends towards the neighbour in azimuth more than towards the one in elevation
    d = 0.3
    az = np.array([[5, 0, 0, 1], [5, d, 0, 1]], np.float32)
    el = np.array([[5, 0, 0, 1], [5, 0, d, 1]], np.float32)
    a = gaussian(R, az, [1, 0], knn_numpy(az, 2), 0.5, 0.1, 10.0)
    b = gaussian(R, el, [1, 0], knn_numpy(el, 2), 0.5, 0.1, 10.0)
    assert a[0] < b[0]
    # a narrow range sigma keeps a depth edge
    ray = np.array([[2, 0, 0, 1], [5, 0, 0, 1]], np.float32)
    out = gaussian(R, ray, [1, 0], knn_numpy(ray, 2), 1.0, 1.0, 0.05)
    assert abs(out[0] - 1.0) <= 0.01 and abs(out[1]) <= 0.01
    # the zenith: finite and inside [0, 1]
    zen = np.array([[0, 0, 5, 1], [0, 0, 6, 1], [0.1, 0, 5, 1]], np.float32)
    out = gaussian(R, zen, [1, 0, 0.5], knn_numpy(zen, 3), 0.3, 0.3, 0.3)
    assert np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0


def test_local_mean_known_answers(R):
    """cpp/tests/test_intensity_local_mean_norm.cpp:25-122"""
    flat = gaussian(R, ARC5, np.full(5, 0.5), knn_numpy(ARC5, 5), 0.3, 0.3, 0.3, mean_min=1e-3)
    assert np.abs(flat - 1.0).max() <= 1e-4
    out = gaussian(R, ARC5, [0.1, 0.1, 1.0, 0.1, 0.1], knn_numpy(ARC5, 5), 0.3, 0.3, 0.3, mean_min=1e-3)
    assert out[2] > 1.0 and out[1] < 1.0 and out[3] < 1.0
    zero = gaussian(R, ARC3, np.zeros(3), knn_numpy(ARC3, 3), 0.3, 0.3, 0.3, mean_min=1e-3)
    assert np.array_equal(bits(zero), bits(np.zeros(3, np.float32)))  # the clamp: exactly 0
    lo = gaussian(R, ARC3, np.full(3, 1e-3 - 1e-6), knn_numpy(ARC3, 3), 0.3, 0.3, 0.3, mean_min=1e-3)
    hi = gaussian(R, ARC3, np.full(3, 1e-3 + 1e-6), knn_numpy(ARC3, 3), 0.3, 0.3, 0.3, mean_min=1e-3)
    assert np.abs(lo - hi).max() <= 1e-2


# ------------------------------------------------------------------------------------------------ exact properties
@pytest.fixture(scope="module")
def small_cloud():
    """2 001 points of the planes cloud with exact neighbours, unit normals that are nearly the planes' (what the angle formulas
    need; the GPU suite takes the library's), and the planted rows"""
    n, k = 2001, 10
    pts, inten, stamps = planes_cloud(n)
    rs = np.random.RandomState(4)
    nrm = np.zeros((n, 4), np.float32)
    for w, axis in enumerate((2, 0, 1)):
        nrm[np.arange(n) % 3 == w, axis] = 1.0
    nrm[:, :3] += rs.normal(0.0, 0.05, (n, 3))
    nrm[:, :3] /= np.linalg.norm(nrm[:, :3], axis=1, keepdims=True)
    covs = np.zeros((n, 16), np.float32)
    knn = knn_numpy(pts, k)
    pts, nrm, covs, knn, regular = plant_rows(pts, nrm, covs, knn)
    return dict(pts=pts, nrm=nrm, knn=knn, inten=inten, regular=regular, n=n, k=k)


def test_angle_filter_properties(R, small_cloud):
    pts, nrm = small_cloud["pts"], small_cloud["nrm"]
    flags = angle_flags(R, pts, nrm, 0.2, 1.2)
    assert set(np.unique(flags)) == {0, 1}  # both outcomes occur (the plane seen from above is nearly all below 0.2 rad ... 1.2 rad)
    for name in ("nan", "inf", "zero_normal", "origin"):
        assert flags[PLANTED[name]] == 0, name
    wide = angle_flags(R, pts, nrm, 0.0, float(np.float32(np.pi) * np.float32(0.5)))
    finite = np.isfinite(pts).all(axis=1)
    ok = finite.copy()
    ok[[PLANTED["zero_normal"], PLANTED["origin"]]] = False
    # [0, pi/2] keeps every finite point with a usable denominator unless rounding puts |cos| above cos(0) = 1
    assert not wide[~ok].any() and wide[ok].mean() > 0.99
    assert np.array_equal(flags, flags & wide)  # narrowing the band only removes
    assert (angle_flags(R, pts, nrm, 0.2, 1.2, f64=True) != flags).mean() < 1e-2  # float32 decides as float64 away from the edges


def test_intensity_correction_properties(R, small_cloud):
    pts, nrm, inten = small_cloud["pts"], small_cloud["nrm"], small_cloud["inten"]
    finite = np.isfinite(pts).all(axis=1)
    # exponent 0: clamp(I * scale) exactly — pow(x, 0) is 1 for every x, NaN included
    got = correct(R, pts, None, inten, 0.0, 1.5, 10.0, 300.0)
    want = np.minimum(np.maximum(inten * np.float32(1.5), np.float32(10.0)), np.float32(300.0))
    assert np.array_equal(bits(got), bits(want))
    # angle_exponent 0 with normals: the bits of the call without normals
    a = correct(R, pts, nrm, inten, 2.0, 0.7, 0.0, 1000.0, 2.0, 0.0)
    b = correct(R, pts, None, inten, 2.0, 0.7, 0.0, 1000.0, 2.0, 0.0)
    assert np.array_equal(bits(a[finite]), bits(b[finite]))
    # a zero normal and a point at the origin: angle factor 1
    c = correct(R, pts, nrm, inten, 2.0, 0.7, 0.0, 1000.0, 2.0, 1.0)
    for name in ("zero_normal", "origin"):
        assert bits(c[PLANTED[name]:PLANTED[name] + 1])[0] == bits(b[PLANTED[name]:PLANTED[name] + 1])[0], name
    # rows the float64 evaluation clamps by a margin come out at the bound exactly
    lo, hi = 40.0, 400.0
    r32 = correct(R, pts, nrm, inten, 2.0, 1.0, lo, hi, 1.0, 1.0)
    free = correct(R, pts, nrm, inten, 2.0, 1.0, -np.inf, np.inf, 1.0, 1.0, f64=True)
    r64 = correct(R, pts, nrm, inten, 2.0, 1.0, lo, hi, 1.0, 1.0, f64=True)
    E_ref = np.abs(r32[finite] - r64[finite]).max()
    assert 0.0 < E_ref <= 1e-3  # float32 rounding of values of up to 400
    above, below = finite & (free > hi + 32 * E_ref), finite & (free < lo - 32 * E_ref)
    assert above.sum() > 10 and below.sum() > 10
    assert (r32[above] == np.float32(hi)).all() and (r32[below] == np.float32(lo)).all()


def test_gaussian_properties(R, small_cloud):
    pts, knn, inten, regular = small_cloud["pts"], small_cloud["knn"], small_cloud["inten"], small_cloud["regular"]
    n, k = knn.shape
    s = (0.1, 0.1, 0.05)
    out, emin, emax = gaussian(R, pts, inten, knn, *s, exponents=True)
    assert emax[regular].max() < 80.0  # no denormal weight among the regular rows
    ref = gaussian(R, pts, inten, knn, *s, f64=True)
    assert np.abs(out[regular] - ref[regular]).max() <= 1e-3
    # every listed neighbour out of reach and the point itself not listed: the own intensity, unchanged
    far = PLANTED["far"]
    assert emin[far] > 200.0 and far not in knn[far]
    assert bits(out[far:far + 1])[0] == bits(inten[far:far + 1])[0]
    org = PLANTED["origin"]
    assert bits(out[org:org + 1])[0] == bits(inten[org:org + 1])[0]
    z = list(PLANTED["zenith"])
    assert np.isfinite(out[z]).all() and out[z].min() >= inten[z].min() and out[z].max() <= inten[z].max()
    # indices outside [0, n) are skipped: the result of the row without them
    for a in PLANTED["out_of_range"]:
        row = knn[a]
        kept = row[(row >= 0) & (row < n)]
        assert len(kept) == k - 2
        alone = np.full((n, k), -1, np.int32)
        alone[a, :len(kept)] = kept
        assert bits(gaussian(R, pts, inten, alone, *s)[a:a + 1])[0] == bits(out[a:a + 1])[0]
    # k_limit on a wider result is the result of the prefix array
    wide = np.concatenate([knn, knn[:, ::-1]], axis=1)
    assert np.array_equal(bits(gaussian(R, pts, inten, wide, *s, k_limit=k)), bits(out))
    assert np.array_equal(bits(gaussian(R, pts, inten, knn, *s, k_limit=3)), bits(gaussian(R, pts, inten, knn[:, :3].copy(), *s)))
    # local-mean normalisation: flat intensity gives 1, zero intensity gives exactly 0
    flat = gaussian(R, pts, np.full(n, 37.5, np.float32), knn, *s, mean_min=1e-3)
    assert np.abs(flat[regular] - 1.0).max() <= 1e-4
    zero = gaussian(R, pts, np.zeros(n, np.float32), knn, *s, mean_min=1e-3)
    assert not bits(zero[regular]).any()
    nrm = gaussian(R, pts, inten, knn, *s, mean_min=1e-3)
    assert np.abs(nrm[regular] - gaussian(R, pts, inten, knn, *s, mean_min=1e-3, f64=True)[regular]).max() <= 1e-4
