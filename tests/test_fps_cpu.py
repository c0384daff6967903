"""Farthest point sampling without a device: the C ABI's exports and argument checks (sp_farthest_point_sampling returns
SP_ERR_INVALID_ARGUMENT before any HIP call), and the CPU restatement of the reference operator (tests/cpp/fps_restate.cpp,
filter/preprocess_operator/farthest_point_sampling_operator.hpp:27-91) on the reference's known answer and on small cases
worked by hand. The GPU suite (tests/test_gpu_fps.py) holds the device to this restatement bit for bit."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.float32(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libfps_restate.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "fps_restate.cpp"), "-o", so])
    R = C.CDLL(so)
    R.fps_first_index.restype = C.c_uint64
    R.fps_first_index.argtypes = [C.c_uint32, C.c_uint64, C.c_int]
    R.fps_restate.restype = None
    R.fps_restate.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    return R


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return build_restatement(tmp_path_factory.mktemp("fps"))


def restate(R, pts, S, first):
    pts = np.ascontiguousarray(pts, np.float32)
    order = np.empty(S, np.uint32)
    d = np.empty(len(pts), np.float32)
    R.fps_restate(pts.ctypes.data_as(C.c_void_p), len(pts), S, first, order.ctypes.data_as(C.c_void_p),
                  d.ctypes.data_as(C.c_void_p))
    return order, d


def test_symbols_exported_and_listed(L):
    from sycl_points_amd import _lib

    for name in ("sp_fps_workspace_bytes", "sp_farthest_point_sampling", "sp_fps_status"):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
    assert "sp_internal_fps" in _lib.INTERNAL_SIGNATURES
    with open(os.path.join(ROOT, "include", "sycl_points_amd.h")) as f:
        assert "sp_internal_fps" not in f.read()
    assert L.sp_fps_workspace_bytes(1000, 10) >= 4000


def test_invalid_arguments_need_no_device(L):
    from sycl_points_amd import _lib

    pts = np.zeros((8, 4), np.float32)
    order = np.zeros(8, np.uint32)
    ws = np.zeros(L.sp_fps_workspace_bytes(8, 8), np.uint8)
    P, O, W = (a.ctypes.data_as(C.c_void_p) for a in (pts, order, ws))
    nb = ws.nbytes
    cases = [
        (P, 0, 1, 0, O, W, nb),            # n == 0
        (None, 8, 2, 0, O, W, nb),         # null points
        (P, 8, 2, 0, None, W, nb),         # null order_out
        (P, 8, 2, 0, O, None, nb),         # null workspace
        (P, 8, 2, 8, O, W, nb),            # first_index >= n
        (P, 8, 0, 0, O, W, nb),            # sampling_num == 0
        (P, 8, 9, 0, O, W, nb),            # sampling_num > n
        (P, 1 << 32, 2, 0, O, W, 1 << 40),  # n >= 2^32
        (P, 8, 2, 0, O, W, nb - 1),        # workspace too small
    ]
    for p, n, s, first, o, w, b in cases:
        assert L.sp_farthest_point_sampling(p, n, s, first, o, None, None, w, b, None) == _lib.SP_ERR_INVALID_ARGUMENT
    # the one-workgroup form takes at most 16384 points, the persistent one 2^21; an unknown form or knob is refused too
    for form, big in ((1, 16385), (3, (1 << 21) + 1), (3 | (2 << 8), 600_000), (3 | (3 << 8), 100), (2 | (17 << 8), 100),
                      (1 | (1 << 8), 100), (4, 8)):
        assert L.sp_internal_fps(form, P, big, 2, 0, O, None, None, W, L.sp_fps_workspace_bytes(big, 2), None) == \
            _lib.SP_ERR_INVALID_ARGUMENT, (form, big)
    assert L.sp_fps_status(None, None) == _lib.SP_ERR_INVALID_ARGUMENT
    assert b"sp_farthest_point_sampling" in L.sp_last_error()


def test_reference_known_answer_unit_square(R):
    """test_preprocess_filter.cpp, FarthestPointSamplingSelectsSpreadPoints: the four corners, seed 1234, three samples: the
    largest pairwise distance of the kept points is sqrt(2)."""
    pts = np.array([[0, 0, 0, 1], [1, 0, 0, 1], [0, 1, 0, 1], [1, 1, 0, 1]], np.float32)
    first = R.fps_first_index(1234, 4, 1)
    order, d = restate(R, pts, 3, first)
    kept = pts[np.unique(order)]
    assert len(kept) == 3
    dmax = max(np.sqrt(((a[:2] - b[:2]) ** 2).sum()) for a, b in itertools.combinations(kept, 2))
    assert np.float32(dmax) == np.float32(np.sqrt(2.0))
    assert order[1] == 3 - order[0]  # the opposite corner comes second


def test_first_index_is_a_uniform_draw(R):
    # std::uniform_int_distribution<size_t>(0, n - 1) on mt19937(1234): in range, and a second draw moves on
    draws = [R.fps_first_index(1234, 1000, k) for k in (1, 2, 3)]
    assert all(0 <= v < 1000 for v in draws) and len(set(draws)) == 3
    assert R.fps_first_index(1234, 1, 1) == 0


def test_lattice_ties_take_the_lowest_index(R):
    # a 1-D lattice 0..4: from 2, both ends are 4 away: index 0 (the first maximum) wins, then 4, then the ties 1 / 3 at 1 -> 1
    pts = np.zeros((5, 4), np.float32)
    pts[:, 0] = np.arange(5)
    order, d = restate(R, pts, 4, 2)
    assert order.tolist() == [2, 0, 4, 1]
    assert d.tolist() == [0.0, 1.0, 0.0, 1.0, 0.0]


def test_duplicates_select_again(R):
    # two distinct positions, five points: once every distance is 0 the first index (0) is selected again and again
    pts = np.array([[0, 0, 0, 1]] * 3 + [[1, 0, 0, 1]] * 2, np.float32)
    order, d = restate(R, pts, 5, 4)
    assert order.tolist() == [4, 0, 0, 0, 0]
    assert not d.any()


def test_nan_point_stays_at_flt_max(R):
    # a NaN coordinate: its distance is NaN, min keeps FLT_MAX, so it is selected as soon as nothing else is farther - and
    # then at every later step, because selecting it updates nothing (every distance to it is NaN)
    pts = np.array([[0, 0, 0, 1], [1, 0, 0, 1], [np.nan, 0, 0, 1], [3, 0, 0, 1]], np.float32)
    order, d = restate(R, pts, 4, 0)
    assert order.tolist() == [0, 2, 2, 2]
    assert d[2] == FLT_MAX and not np.isnan(d).any()


def test_w_component_counts(R):
    # w enters the distance (dot<4>): point 1 differs from point 0 in w only and is the farthest from it
    pts = np.array([[0, 0, 0, 1], [0, 0, 0, 5], [1, 0, 0, 1]], np.float32)
    order, d = restate(R, pts, 2, 0)
    assert order.tolist() == [0, 1]
    assert d.tolist() == [0.0, 16.0, 1.0]


def test_fma_chain_is_not_a_plain_sum(R):
    # the restatement rounds as fma(dw,dw, fma(dz,dz, fma(dy,dy, dx*dx))): check one distance against that chain in float64
    rs = np.random.RandomState(3)
    pts = rs.uniform(-10, 10, (2, 4)).astype(np.float32)
    _, d = restate(R, pts, 2, 0)
    dv = (pts[1] - pts[0]).astype(np.float32)
    acc = np.float32(0.0)
    for c in range(4):
        acc = np.float32(np.float64(dv[c]) * np.float64(dv[c]) + np.float64(acc))  # one rounding per step: fmaf
    assert d[1] == acc
