"""OutlierRemoval and the intensity z-score without a device: the C ABI's exports and argument checks (sp_outlier_statistical_flags,
sp_outlier_radius_flags and sp_intensity_zscore return their errors before any HIP call, the z-score with the reference's texts),
the resource report of csrc/outlier.hip, the Python mirror's names, and the CPU restatement of the three formulas
(tests/cpp/outlier_restate.cpp) on hand-computed answers.

The helpers here (the restatement's wrappers) are the GPU suite's too (tests/test_gpu_outlier.py)."""
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
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "liboutlier_restate.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "outlier_restate.cpp"), "-o", so])
    R = C.CDLL(so)
    for name in ("outlier_statistical_restate", "outlier_statistical_f64"):
        getattr(R, name).restype = None
        getattr(R, name).argtypes = [_vp, _u64, _u64, _u64, _f, _vp, _vp, _vp]
    R.outlier_radius_restate.restype = None
    R.outlier_radius_restate.argtypes = [_vp, _u64, _u64, _u64, _f, _vp]
    for name in ("intensity_zscore_restate", "intensity_zscore_f64"):
        getattr(R, name).restype = None
        getattr(R, name).argtypes = [_vp, _vp, _u64, _u64, _u64, _f, _vp]
    return R


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return build_restatement(tmp_path_factory.mktemp("outlier"))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def statistical(R, d2, k_use, mul, f64=False):
    """(means, stats = [g, var, thr, n], flags) of rows of squared distances"""
    d2 = np.ascontiguousarray(d2, np.float32)
    n, ks = d2.shape
    T = np.float64 if f64 else np.float32
    mean, stats, flags = np.empty(n, T), np.empty(4, T), np.full(n, 7, np.uint8)
    (R.outlier_statistical_f64 if f64 else R.outlier_statistical_restate)(_ptr(d2), n, ks, k_use, mul, _ptr(mean), _ptr(stats), _ptr(flags))
    return mean, stats, flags


def radius_flags(R, d2, column, radius):
    d2 = np.ascontiguousarray(d2, np.float32)
    n, ks = d2.shape
    flags = np.full(n, 7, np.uint8)
    R.outlier_radius_restate(_ptr(d2), n, ks, column, radius, _ptr(flags))
    return flags


def zscore(R, inten, knn, k_use=0, sigma_min=0.01, f64=False):
    inten = np.ascontiguousarray(inten, np.float32)
    knn = np.ascontiguousarray(knn, np.int32)
    n, ks = knn.shape
    out = np.empty(n, np.float64 if f64 else np.float32)
    (R.intensity_zscore_f64 if f64 else R.intensity_zscore_restate)(_ptr(inten), _ptr(knn), n, ks, k_use or ks, sigma_min, _ptr(out))
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


NEW_SYMBOLS = ("sp_outlier_workspace_bytes", "sp_outlier_statistical_flags", "sp_outlier_radius_flags", "sp_intensity_zscore")


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbols_exported_and_listed(L):
    from sycl_points_amd import _lib

    with open(os.path.join(ROOT, "include", "sycl_points_amd.h")) as f:
        hdr = f.read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
        assert name + "(" in hdr
    assert hasattr(L, "sp_compact_by_flags_multi")  # the compaction both filters hand over to
    assert L.sp_abi_version() == 7
    assert re.search(r"#define SP_ABI_VERSION 7\b", hdr)


def test_facade_headers_are_there():
    for name in ("outlier_removal_filter", "intensity_zscore"):
        assert os.path.exists(os.path.join(ROOT, "include", "sycl_points", "algorithms", "filter", name + ".hpp"))
    with open(os.path.join(ROOT, "include", "sycl_points", "amd", "features.hpp")) as f:
        text = f.read()
    assert "class OutlierRemoval" in text and "namespace intensity_zscore" in text


def test_python_mirror_is_there():
    import sycl_points_amd.api as api

    assert callable(api.intensity_zscore)
    for name in ("statistical", "radius", "get_flags", "calculate_indices"):
        assert callable(getattr(api.OutlierRemoval, name))


def test_invalid_arguments_need_no_device(L):
    from sycl_points_amd import _lib

    a = np.zeros((8, 16), np.float32)
    b = np.zeros((8, 16), np.float32)
    ws = np.zeros(1 << 14, np.uint8)
    P, Q, W = _ptr(a), _ptr(b), _ptr(ws)
    RT, IA = _lib.SP_ERR_RUNTIME, _lib.SP_ERR_INVALID_ARGUMENT
    need = L.sp_outlier_workspace_bytes(8)
    assert 0 < need <= ws.nbytes and L.sp_outlier_workspace_bytes(1 << 20) <= 1 << 16  # a few partial sums, whatever n

    def stat(d2=P, n=8, ks=10, ku=10, flags=Q, mean=Q, stats=Q, w=W, wb=need):
        return L.sp_outlier_statistical_flags(d2, n, ks, ku, 1.0, flags, mean, stats, w, wb, None)

    for kw in (dict(ku=0), dict(ku=11), dict(ks=0, ku=0), dict(d2=None), dict(flags=None), dict(mean=None), dict(stats=None),
               dict(w=None), dict(wb=need - 1), dict(wb=0), dict(n=1 << 31)):
        assert stat(**kw) == IA, kw
        assert b"sp_outlier_statistical_flags" in L.sp_last_error(), (kw, L.sp_last_error())
    assert stat(n=0, d2=None, flags=None, mean=None, stats=None, w=None, wb=0, ku=0) == 0

    def rad(d2=P, n=8, ks=4, col=3, flags=Q):
        return L.sp_outlier_radius_flags(d2, n, ks, col, 0.5, flags, None)

    for kw in (dict(col=4), dict(col=9), dict(ks=0, col=0), dict(d2=None), dict(flags=None), dict(n=1 << 31)):
        assert rad(**kw) == IA, kw
        assert b"sp_outlier_radius_flags" in L.sp_last_error(), (kw, L.sp_last_error())
    assert rad(n=0, d2=None, flags=None, col=7) == 0

    idx = np.zeros((8, 10), np.int32)
    K = _ptr(idx)

    def zs(i_in=P, knn=K, n=8, ks=10, ku=10, out=Q):
        return L.sp_intensity_zscore(i_in, knn, n, ks, ku, 0.01, out, None)

    for kw, code, text in [(dict(i_in=None), RT, b"[intensity_zscore::compute] Intensity field not found"),
                           (dict(ku=2), RT, b"[intensity_zscore::compute] neighbors.k must be >= 3"),
                           (dict(ks=2, ku=2), RT, b"[intensity_zscore::compute] neighbors.k must be >= 3"),
                           (dict(ku=0), RT, b"[intensity_zscore::compute] neighbors.k must be >= 3"),
                           (dict(i_in=None, ku=1), RT, b"[intensity_zscore::compute] Intensity field not found"),  # the reference's order
                           (dict(out=P), IA, b"intensities_out must not be intensities_in"),
                           (dict(ku=11), IA, b"sp_intensity_zscore"), (dict(knn=None), IA, b"sp_intensity_zscore"),
                           (dict(out=None), IA, b"sp_intensity_zscore"), (dict(n=1 << 31), IA, b"sp_intensity_zscore")]:
        assert zs(**kw) == code, kw
        assert L.sp_last_error() == text or text in L.sp_last_error(), (kw, L.sp_last_error())
    assert zs(n=0, i_in=None, knn=None, out=None, ku=0) == 0  # an empty cloud: before any check


def test_resource_report_has_no_scratch(L):
    path = os.path.join(ROOT, "sycl_points_amd", "lib", "outlier.resources.txt")
    with open(path) as f:
        rows = f.read().splitlines()
    for kernel, count in (("mean_kernel", 2), ("variance_kernel", 1), ("flags_kernel", 1), ("radius_flags_kernel", 1), ("zscore_kernel", 2)):
        mine = [r for r in rows if kernel in r and (kernel != "flags_kernel" or "radius_" not in r)]
        assert len(mine) == count, (kernel, mine)
        for r in mine:
            assert re.search(r"VGPRs Spill: 0\b", r) and re.search(r"ScratchSize \[bytes/lane\]: 0\b", r), r
    assert len(rows) == 7


# ------------------------------------------------------------------------------------------------ hand-computed answers
def test_statistical_six_points_by_hand(R):
    """rows of stride 3 of which two entries count: the means are 0, 0, 0, 4, 4, 4, so g = 2, the variance is 4, the deviation 2 and
    thr = 2 + 2 mul, every value exact in float. mul = 0.5: thr = 3 removes the three rows at 4; mul = 1: thr = 4 and 4 > 4 is
    false, nothing goes (the comparison is strict); the third column never counts."""
    d2 = np.array([[0, 0, 99], [0, 0, 99], [0, 0, 99], [0, 8, 99], [1, 7, 99], [3, 5, 99]], np.float32)
    for f64 in (False, True):
        mean, stats, flags = statistical(R, d2, 2, 0.5, f64=f64)
        assert mean.tolist() == [0, 0, 0, 4, 4, 4]
        assert stats.tolist() == [2.0, 4.0, 3.0, 6.0]
        assert flags.tolist() == [1, 1, 1, 0, 0, 0]
        mean, stats, flags = statistical(R, d2, 2, 1.0, f64=f64)
        assert stats.tolist() == [2.0, 4.0, 4.0, 6.0] and flags.tolist() == [1] * 6
        mean, stats, flags = statistical(R, d2, 3, 0.5, f64=f64)  # all three columns
        third = 107 / 3 if f64 else float(np.float32(107) / np.float32(3))
        assert mean.tolist() == [33, 33, 33, third, third, third]
        assert abs(stats[0] - (99 + 107) / 6.0) < 1e-5
    # a row with FLT_MAX padding sums to inf (two paddings) or to a huge finite value (one): literal, and such a row is removed
    pad = np.array([[0, 1, 2], [0, 1, 2], [0, 1, FLT_MAX], [0, FLT_MAX, FLT_MAX]], np.float32)
    mean, stats, flags = statistical(R, pad, 3, 1.0)
    assert mean[0] == 1.0 and np.isfinite(mean[2]) and mean[2] > 1e38 and np.isinf(mean[3])
    assert np.isinf(stats[0]) and np.isnan(stats[2])  # inf - inf in the variance: nothing is above a NaN threshold
    assert flags.tolist() == [1, 1, 1, 1]


def test_radius_column_rule(R):
    """column min_k of rows of min_k + 1 entries, squared distance against the radius ITSELF: with radius 0.5 a squared distance of
    0.3 (a distance of 0.548 > 0.5, between r^2 = 0.25 and r) stays, which a comparison of distances would remove; 0.5 is not
    above 0.5; 0.6 goes. The columns before min_k never count."""
    d2 = np.array([[0, 0.01, 0.2], [0, 0.01, 0.3], [0, 0.01, 0.5], [0, 0.01, 0.6], [0, 9.0, 0.1], [0, 0.01, FLT_MAX]], np.float32)
    assert radius_flags(R, d2, 2, 0.5).tolist() == [1, 1, 1, 0, 1, 0]
    assert radius_flags(R, d2, 2, 0.25).tolist() == [1, 0, 0, 0, 1, 0]  # what r^2 as the threshold would give
    assert radius_flags(R, d2, 1, 0.5).tolist() == [1, 1, 1, 1, 0, 1]


def test_zscore_known_answers(R):
    knn = np.array([[0, 1, 2], [1, 0, 2], [2, 1, 0]], np.int32)
    # a constant neighbourhood: sigma = 0 < sigma_min, the result is exactly 0
    assert not bits(zscore(R, [5.5, 5.5, 5.5], knn)).any()
    # k = 3 by hand: I = 1, 2, 3: S = 6, Q = 14, mean = 2, var = 14/3 - 4 = 2/3, z = (I - 2) / sqrt(2/3)
    want = (np.array([1.0, 2.0, 3.0]) - 2.0) / np.sqrt(2.0 / 3.0)
    assert np.abs(zscore(R, [1, 2, 3], knn, f64=True) - want).max() < 1e-14
    assert np.abs(zscore(R, [1, 2, 3], knn) - want).max() < 1e-6
    # I = 1, 1, 4: mean 2, Q / 3 = 6, var 2: exact up to the final square root and division
    got = zscore(R, [1, 1, 4], knn)
    assert np.array_equal(bits(got), bits(np.array([-1, -1, 2], np.float32) / np.sqrt(np.float32(2))))
    # k = 4, I = 0, 0, 2s, 2s with s = 2^-6: mean = s, var = s^2, sigma = s, all exact. sigma_min = s: s < s is false, z = (I - s) / s
    # = -1, -1, 1, 1; the next float above s as sigma_min: 0
    s = np.float32(2.0 ** -6)
    knn4 = np.array([[0, 1, 2, 3], [1, 0, 2, 3], [2, 3, 0, 1], [3, 2, 1, 0]], np.int32)
    inten = np.array([0, 0, 2 * s, 2 * s], np.float32)
    for f64 in (False, True):
        assert zscore(R, inten, knn4, sigma_min=float(s), f64=f64).tolist() == [-1, -1, 1, 1]
        assert zscore(R, inten, knn4, sigma_min=float(np.nextafter(s, np.float32(1))), f64=f64).tolist() == [0, 0, 0, 0]
        assert zscore(R, inten, knn4, sigma_min=float(np.nextafter(s, np.float32(0))), f64=f64).tolist() == [-1, -1, 1, 1]
    # an index outside [0, n) adds nothing and the divisor stays k_use; k_use takes a prefix of a wider row
    wide = np.array([[0, 1, 2, 3, -1, 4, 7], [1, 0, 2, 3, 2 ** 31 - 1, 0, 0], [2, 3, 0, 1, -7, 0, 0], [3, 2, 1, 0, 4, 0, 0]], np.int32)
    base = zscore(R, inten, knn4, sigma_min=1e-3)
    assert np.array_equal(bits(zscore(R, inten, wide, k_use=4, sigma_min=1e-3)), bits(base))
    got5 = zscore(R, inten, wide, k_use=5, sigma_min=1e-3)  # four neighbours over a divisor of 5: mean 4s/5, var 8s^2/5 - 16s^2/25
    want5 = (inten.astype(np.float64) - 0.8 * s) / np.sqrt((1.6 - 0.64) * float(s) ** 2)
    assert np.abs(got5 - want5).max() < 1e-6
    # a NaN among the neighbours: fmax drops the NaN variance, sigma = 0, the result is 0
    assert not bits(zscore(R, [1, np.nan, 3], knn)).any()
