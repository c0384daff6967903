"""Farthest point sampling on the device (sp_farthest_point_sampling, sp_internal_fps, api.farthest_point_sampling and the C++
facade's PreprocessFilter::farthest_point_sampling) against the CPU restatement of the reference operator
(tests/cpp/fps_restate.cpp; filter/preprocess_operator/farthest_point_sampling_operator.hpp:27-91): the order of the samples
and every point's final minimum distance bit for bit, in every form and by the library's own choice."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.float32(np.finfo(np.float32).max)
ONE_WG_CAP = 16384
PERSIST_CAP = 1 << 21


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("fps")), "libfps_restate.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "fps_restate.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.fps_first_index.restype = C.c_uint64
    lib.fps_first_index.argtypes = [C.c_uint32, C.c_uint64, C.c_int]
    lib.fps_restate.restype = None
    lib.fps_restate.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


def restate(R, pts, S, first):
    pts = np.ascontiguousarray(pts, np.float32)
    order = np.empty(S, np.uint32)
    d = np.empty(len(pts), np.float32)
    R.fps_restate(pts.ctypes.data_as(C.c_void_p), len(pts), S, first, order.ctypes.data_as(C.c_void_p),
                  d.ctypes.data_as(C.c_void_p))
    return order, d


def uniform(n, seed=1234):
    from sycl_points_amd.synthetic import Mt19937Cloud

    return np.ascontiguousarray(Mt19937Cloud(seed).uniform_points(n, 10.0), np.float32)


def surface(n, seed=5):
    # a scan-like cloud: a ground plane and a wall, points on the surfaces only, with a little noise
    rs = np.random.RandomState(seed)
    m = n // 2
    ground = np.c_[rs.uniform(-30, 30, m), rs.uniform(-30, 30, m), rs.normal(0, 0.02, m)]
    wall = np.c_[rs.uniform(-30, 30, n - m), np.full(n - m, 12.0) + rs.normal(0, 0.02, n - m), rs.uniform(0, 5, n - m)]
    return np.c_[np.r_[ground, wall], np.ones(n)].astype(np.float32)


def lattice(side):
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return np.c_[g, np.ones(len(g))].astype(np.float32)  # integer coordinates: exact ties everywhere


def run(sp, pts, S, first, form):
    r = sp.farthest_point_sampling(torch.from_numpy(pts).cuda(), S, first, form=form)
    return r.order.cpu().numpy().view(np.uint32), r.flags.cpu().numpy(), r.min_d2.cpu().numpy()


def check_against(R, sp, pts, S, first, forms):
    ref_order, ref_d = restate(R, pts, S, first)
    ref_flags = np.zeros(len(pts), np.uint8)
    ref_flags[ref_order] = 1
    for form in forms:
        order, flags, d = run(sp, pts, S, first, form)
        assert np.array_equal(order, ref_order), (form, np.flatnonzero(order != ref_order)[:5])
        assert np.array_equal(d.view(np.uint32), ref_d.view(np.uint32)), form
        assert np.array_equal(flags, ref_flags), form


def forms_for(n):
    return ([None] + (["one_workgroup"] if n <= ONE_WG_CAP else []) + (["persistent"] if n <= PERSIST_CAP else [])
            + ["per_sample"])


CASES = [(2, 1), (2, 2), (64, 63), (64, 64), (1000, 999), (1000, 1000), (6000, 4096), (6000, 5999), (100_000, 4096),
         (1_048_576, 512)]


@pytest.mark.parametrize("n,S", CASES)
def test_uniform_bit_identical(sp, R, n, S):
    pts = uniform(n)
    first = int(R.fps_first_index(1234, n, 1))
    check_against(R, sp, pts, S, first, forms_for(n))


@pytest.mark.parametrize("n", [1023, 1024, 1025, 8191, 8192, 8193, ONE_WG_CAP - 1, ONE_WG_CAP, ONE_WG_CAP + 1])
def test_capacity_boundaries(sp, R, n):
    pts = uniform(n, seed=n)
    check_against(R, sp, pts, 1000, n // 3, forms_for(n))


@pytest.mark.parametrize("n,S", [(PERSIST_CAP, 200), (PERSIST_CAP + 1, 100)])
def test_persistent_capacity_boundary(sp, R, n, S):
    check_against(R, sp, uniform(n, seed=7), S, n - 1, forms_for(n))


@pytest.mark.parametrize("n", [70_000, 300_000])
def test_persistent_points_per_lane(sp, R, n):
    """Every grid shape of the persistent form (1, 2, 4, 8 points per lane: 69 to 9 workgroups at 70 k) gives the same bits."""
    from sycl_points_amd import _lib

    L = _lib.lib()
    pts_np = surface(n, seed=n)
    ref_order, ref_d = restate(R, pts_np, 700, 3)
    pts = torch.from_numpy(pts_np).cuda()
    nb = L.sp_fps_workspace_bytes(n, 700)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    order = torch.empty(700, dtype=torch.int32, device="cuda")
    d = torch.empty(n, dtype=torch.float32, device="cuda")
    for per in (1, 2, 4, 8):
        if -(-n // (1024 * per)) > 256:
            continue
        order.zero_()
        rc = L.sp_internal_fps(_lib.FPS_FORM["persistent"] | (per << 8), C.c_void_p(pts.data_ptr()), n, 700, 3,
                               C.c_void_p(order.data_ptr()), None, C.c_void_p(d.data_ptr()), C.c_void_p(ws.data_ptr()), nb,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        assert L.sp_fps_status(C.c_void_p(ws.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        assert np.array_equal(order.cpu().numpy().view(np.uint32), ref_order), per
        assert np.array_equal(d.cpu().numpy().view(np.uint32), ref_d.view(np.uint32)), per


@pytest.mark.parametrize("n,S", [(6000, 2000), (50_000, 1500)])
def test_surface_bit_identical(sp, R, n, S):
    check_against(R, sp, surface(n), S, 17, forms_for(n))


@pytest.mark.parametrize("side,S", [(12, 1728), (20, 3000), (40, 2000)])
def test_lattice_ties(sp, R, side, S):
    pts = lattice(side)
    check_against(R, sp, pts, S, len(pts) // 2, forms_for(len(pts)))


def test_one_workgroup_form_refuses_above_capacity(sp):
    with pytest.raises(sp.SpError) as e:
        run(sp, uniform(ONE_WG_CAP + 1), 10, 0, "one_workgroup")
    assert e.value.code == 1


def test_duplicates_select_again(sp, R):
    base = uniform(50)
    pts = np.repeat(base, 20, axis=0)  # 1000 points, 50 positions
    check_against(R, sp, pts, 200, 7, forms_for(len(pts)))
    order, flags, d = run(sp, pts, 200, 7, None)
    assert not d.any() and int(flags.sum()) < 200  # every distance is 0: the first index comes again


def test_nan_point_selected_again(sp, R):
    pts = uniform(3000)
    pts[1234, 1] = np.nan
    check_against(R, sp, pts, 300, 0, forms_for(len(pts)))
    order, _, d = run(sp, pts, 300, 0, None)
    k = int(np.flatnonzero(order == 1234)[0])
    assert (order[k:] == 1234).all() and d[1234] == FLT_MAX and not np.isnan(d).any()


def test_sampling_num_zero_and_one(sp, R):
    pts = uniform(100)
    with pytest.raises(sp.SpError) as e:  # the ABI asks for at least one sample; the facade keeps the first point itself
        sp.farthest_point_sampling(torch.from_numpy(pts).cuda(), 0, 3)
    assert e.value.code == 1
    for form in forms_for(100):
        order, flags, d = run(sp, pts, 1, 42, form)
        assert order.tolist() == [42] and np.flatnonzero(flags).tolist() == [42] and (d == FLT_MAX).all()


def test_graph_capture_and_replay(sp, R):
    from sycl_points_amd import _lib

    L = _lib.lib()
    n, S = 20_000, 300
    pts_np = uniform(n, seed=3)
    ref_order, ref_d = restate(R, pts_np, S, 5)
    pts = torch.from_numpy(pts_np).cuda()
    order = torch.zeros(S, dtype=torch.int32, device="cuda")
    d = torch.zeros(n, dtype=torch.float32, device="cuda")
    nb = L.sp_fps_workspace_bytes(n, S)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = L.sp_internal_fps(_lib.FPS_FORM["per_sample"], C.c_void_p(pts.data_ptr()), n, S, 5, C.c_void_p(order.data_ptr()),
                               None, C.c_void_p(d.data_ptr()), C.c_void_p(ws.data_ptr()), nb,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    for _ in range(2):
        order.zero_()
        d.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(order.cpu().numpy().view(np.uint32), ref_order)
        assert np.array_equal(d.cpu().numpy().view(np.uint32), ref_d.view(np.uint32))


def test_two_streams_at_once(sp, R):
    """Two clouds large enough for the persistent form, on two streams at once: the persistent-launch guard lets one of them run
    persistent and sends the other (while the first may still run) to the per-sample form; both orders are right."""
    a_np, b_np = uniform(300_000, seed=21), uniform(200_000, seed=22)
    ref_a, _ = restate(R, a_np, 2000, 9)
    ref_b, _ = restate(R, b_np, 2000, 10)
    from sycl_points_amd import _lib

    L = _lib.lib()
    bufs = []
    for pts_np in (a_np, b_np):
        n = len(pts_np)
        nb = L.sp_fps_workspace_bytes(n, 2000)
        bufs.append((torch.from_numpy(pts_np).cuda(), n, torch.empty(2000, dtype=torch.int32, device="cuda"),
                     torch.empty(nb, dtype=torch.uint8, device="cuda"), nb))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for (P, n, order, ws, nb), st, first in zip(bufs, streams, (9, 10)):  # both enqueued before either is waited for
        assert L.sp_farthest_point_sampling(C.c_void_p(P.data_ptr()), n, 2000, first, C.c_void_p(order.data_ptr()), None, None,
                                            C.c_void_p(ws.data_ptr()), nb, C.c_void_p(st.cuda_stream)) == 0
    for (P, n, order, ws, nb), st in zip(bufs, streams):
        assert L.sp_fps_status(C.c_void_p(ws.data_ptr()), C.c_void_p(st.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bufs[0][2].cpu().numpy().view(np.uint32), ref_a)
    assert np.array_equal(bufs[1][2].cpu().numpy().view(np.uint32), ref_b)


def test_fps_kernels_do_not_spill():
    path = os.path.join(ROOT, "sycl_points_amd", "lib", "fps.resources.txt")
    with open(path) as f:
        rows = [r for r in f.read().splitlines() if "fps" in r]
    assert len(rows) >= 8, rows
    for r in rows:
        assert re.search(r"VGPRs Spill: 0\b", r) and re.search(r"ScratchSize \[bytes/lane\]: 0\b", r), r


def test_cpp_facade(sp):
    """tests/cpp/test_fps.cpp, built with tests/cpp/Makefile's flags and libraries (the Makefile is not changed)."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(cpp, "test_fps")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    lib = os.path.join(ROOT, "sycl_points_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++20", f"-I{ROOT}/include", f"-I{rocm}/include", "-D__HIP_PLATFORM_AMD__", "-Wall",
                           "-Wno-unused-value", "-Wno-unused-result", os.path.join(cpp, "test_fps.cpp"), "-o", exe,
                           f"-L{lib}", "-lsycl_points_amd", f"-Wl,-rpath,{lib}", f"-L{rocm}/lib", "-lamdhip64",
                           f"-Wl,-rpath,{rocm}/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
