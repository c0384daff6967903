"""Weighted and mixed random sampling on the device (sp_weight_check, sp_weighted_sample_flags, sp_uniform_fill_flags, their
api mirrors and the C++ facade's PreprocessFilter::weighted_random_sampling / mixed_random_sampling) against the CPU restatement
of the reference operators (tests/cpp/sampling_restate.cpp): flags bit for bit. A device key may differ from the restatement's
by 2 ulp (the logarithm), so every random case first asserts that the restatement's m-th and (m + 1)-th largest
keys are more than 8 ulp apart; the tie cases use identical (u, w) pairs only, which tie exactly on both sides."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_sampling_cpu import (MARGIN_ULP, RANDOM_CASES, TIE_CASES, TILE, U9, build_restatement, draws, heap_select, keys_of,
                               mixed_restate, random_case, random_weights, threshold_gap_ulp, uniform_positions)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return build_restatement(tmp_path_factory.mktemp("sampling"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_flags(sp, w, u, m):
    flags, count = sp.weighted_sample_flags(dev(w), dev(u), m)
    flags = flags.cpu().numpy()
    assert count == int(flags.sum()) == min(m, int((w > 0).sum()))
    return flags


@pytest.mark.parametrize("n,seed", RANDOM_CASES)
def test_random_weights_bit_identical(sp, R, n, seed):
    w, u, keys, ms = random_case(R, n, seed)
    assert sp.weight_check(dev(w)) == (int((w > 0).sum()), None)
    for m in ms:
        gap = threshold_gap_ulp(keys, m)
        assert gap is None or gap > MARGIN_ULP, (m, gap)
        ref = heap_select(R, keys, m)
        got = device_flags(sp, w, u, m)
        assert np.array_equal(got, ref), (m, np.flatnonzero(got != ref)[:8])


def test_weight_check_reports_the_first_bad_weight(sp):
    w = random_weights(5000, 1)
    assert sp.weight_check(dev(w)) == (int((w > 0).sum()), None)
    for bad in (np.nan, np.inf, -np.inf, -1e-30):
        v = w.copy()
        v[[4097, 1300, 4999]] = bad
        positive, first = sp.weight_check(dev(v))
        assert first == 1300 and positive == int((v > 0).sum())
    v = w.copy()
    v[0] = -0.0  # -0 is not < 0 and not > 0
    assert sp.weight_check(dev(v)) == (int((w[1:] > 0).sum()), None)
    assert sp.weight_check(dev(np.zeros(70, np.float32))) == (0, None)


def spread(u, n, stride):
    """The hand-made case's points at indices 0, stride, 2 * stride, ... of a cloud of n points; the others have no weight."""
    w = np.zeros(n, np.float32)
    idx = np.arange(len(u)) * stride
    w[idx] = 1.0
    return w, idx


@pytest.mark.parametrize("stride", [1, 64, TILE, TILE + 1])
@pytest.mark.parametrize("u,m,kept", TIE_CASES)
def test_crafted_ties(sp, R, u, m, kept, stride):
    """The CPU file's hand-made cases through the device, next to each other and one per wave / per tile."""
    u = np.array(u, np.float32)
    w, idx = spread(u, (len(u) - 1) * stride + 3, stride)
    assert np.flatnonzero(device_flags(sp, w, u, m)).tolist() == idx[kept].tolist()


@pytest.mark.parametrize("n", [200, 3 * TILE + 5])
@pytest.mark.parametrize("weight", [1.0, 1e-40])
def test_many_ties_every_m(sp, R, n, weight):
    """u from {0.1 .. 0.9} and one weight for all: a ninth of the keys tie at every threshold; 1e-40 makes every key -inf."""
    rs = np.random.RandomState(n)
    w = np.full(n, weight, np.float32)
    w[rs.uniform(size=n) < 0.3] = 0.0
    positive = int((w > 0).sum())
    u = U9[rs.randint(0, 9, positive)]
    keys = keys_of(R, w, u)
    assert np.isneginf(keys[w > 0]).all() == (weight < 1e-39)
    for m in sorted({1, 2, 7, positive // 3, positive // 2, positive - 1, positive}):
        ref = heap_select(R, keys, m)
        got = device_flags(sp, w, u, m)
        assert np.array_equal(got, ref), (m, np.flatnonzero(got != ref)[:8])


def test_fewer_positive_weights_than_m(sp, R):
    w = np.zeros(3000, np.float32)
    w[[5, 1023, 1024, 2999]] = [1.0, 2.0, 0.5, 3.0]
    u = np.array([0.5, 0.5, 0.5, 0.5], np.float32)
    for m in (4, 5, 2000, 3000):
        assert np.flatnonzero(device_flags(sp, w, u, m)).tolist() == [5, 1023, 1024, 2999]


def run_mixed(sp, R, seed, w, m, ratio):
    """mixed_random_sampling as the facade runs it, through the api mirrors: the draws and positions of the restatement's
    exports, the flags by the device."""
    n = len(w)
    positive, bad = sp.weight_check(dev(w))
    assert bad is None
    target = int(np.floor(m * np.float64(np.float32(ratio))))
    selected = min(target, positive)
    drawn = positive if target else 0
    if selected:
        flags, count = sp.weighted_sample_flags(dev(w), dev(draws(R, seed, positive)), target)
        assert count == selected
    else:
        flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
    Rn = n - selected
    U = min(m - selected, Rn)
    if U:
        pos = np.sort(uniform_positions(R, seed, drawn, Rn, U)).astype(np.int64)
        sp.uniform_fill_flags(flags, torch.from_numpy(pos))
    return flags.cpu().numpy(), selected, U


MIXED_CASES = [
    # n, m, ratio, share of zero weights
    (300, 100, 0.8, 0.2),
    (300, 100, 0.0, 0.2),           # weighted_target == 0: no weighted draw
    (300, 299, 0.1, 0.2),           # U = R - 1: all but one of the remaining points (N > sampling_num keeps U below R)
    (5000, 1000, 0.8, 0.97),        # positive_count < weighted_target
    (3 * TILE + 1, 2 * TILE, 0.5, 0.5),
    (64, 63, 1.0, 0.9),             # ratio 1 with few positive weights: the uniform part fills nearly everything
]


@pytest.mark.parametrize("n,m,ratio,zero_share", MIXED_CASES)
def test_mixed_end_to_end(sp, R, n, m, ratio, zero_share):
    seed = n + m
    w = random_weights(n, seed, zero_share)
    target = int(np.floor(m * np.float64(np.float32(ratio))))
    if target:
        gap = threshold_gap_ulp(keys_of(R, w, draws(R, seed, int((w > 0).sum()))), target)
        assert gap is None or gap > MARGIN_ULP, gap
    rc, ref = mixed_restate(R, seed, w, m, float(ratio))
    assert rc == 0
    got, selected, U = run_mixed(sp, R, seed, w, m, ratio)
    assert int(got.sum()) == selected + U == m
    assert np.array_equal(got, ref), np.flatnonzero(got != ref)[:8]


def test_uniform_fill_positions(sp):
    """Positions at 0, at R - 1 and on both sides of tile boundaries, with flagged points in between; a position past R - 1
    selects nothing."""
    n = 3 * TILE + 7
    rs = np.random.RandomState(2)
    flags = (rs.uniform(size=n) < 0.4).astype(np.uint8)
    flags[[0, TILE - 1, TILE, n - 1]] = [1, 0, 0, 0]
    open_idx = np.flatnonzero(flags == 0)
    Rn = len(open_idx)
    at = lambda i: int(np.searchsorted(open_idx, i))  # noqa: E731  (the position of open point i)
    pos = sorted({0, 1, at(TILE - 1), at(TILE), at(2 * TILE - 3), at(2 * TILE + 2), Rn - 2, Rn - 1})
    want = flags.copy()
    want[open_idx[pos]] = 1
    got = sp.uniform_fill_flags(dev(flags), torch.tensor(pos + [Rn, Rn + 5])).cpu().numpy()
    assert np.array_equal(got, want)
    every = sp.uniform_fill_flags(dev(flags), torch.arange(Rn)).cpu().numpy()  # U == R
    assert every.all()


def _raw_call(L, w, u, m, flags, ws, nb, stream):
    return L.sp_weighted_sample_flags(C.c_void_p(w.data_ptr()), C.c_void_p(u.data_ptr()), w.numel(), m,
                                      C.c_void_p(flags.data_ptr()), None, C.c_void_p(ws.data_ptr()), nb, C.c_void_p(stream))


def test_graph_capture_and_replay(sp, R):
    """One capture of the weighted selection and of the uniform fill behind it, replayed on new weights and draws: only the
    given stream is used, and nothing is decided on the host."""
    from sycl_points_amd import _lib

    L = _lib.lib()
    n, m = 4097, 500
    w, u, flags = (torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"))
    pos = torch.tensor([0, 3, n - m - 1], dtype=torch.int32, device="cuda")
    nb, nb2 = L.sp_weighted_sample_workspace_bytes(n), L.sp_uniform_fill_workspace_bytes(n)
    ws, ws2 = torch.empty(nb, dtype=torch.uint8, device="cuda"), torch.empty(nb2, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        rc = _raw_call(L, w, u, m, flags, ws, nb, st)
        rc2 = L.sp_uniform_fill_flags(C.c_void_p(flags.data_ptr()), n, C.c_void_p(pos.data_ptr()), 3, C.c_void_p(ws2.data_ptr()),
                                      nb2, C.c_void_p(st))
    assert rc == 0 and rc2 == 0
    for seed in (9, 12):
        w_np, u_np, keys, _ = random_case(R, n, seed)
        gap = threshold_gap_ulp(keys, m)
        assert gap is not None and gap > MARGIN_ULP
        w.copy_(dev(w_np))
        u[:len(u_np)].copy_(dev(u_np))
        flags.fill_(9)
        g.replay()
        torch.cuda.synchronize()
        ref = heap_select(R, keys, m)
        open_idx = np.flatnonzero(ref == 0)
        ref[open_idx[[0, 3, n - m - 1]]] = 1
        assert np.array_equal(flags.cpu().numpy(), ref)


def test_two_streams_at_once(sp, R):
    from sycl_points_amd import _lib

    L = _lib.lib()
    jobs = []
    for n, seed, m in ((69_001, 21, 1000), (50_000, 22, 700)):
        w_np = random_weights(n, seed)
        u_np = draws(R, seed, int((w_np > 0).sum()))
        keys = keys_of(R, w_np, u_np)
        assert threshold_gap_ulp(keys, m) > MARGIN_ULP
        nb = L.sp_weighted_sample_workspace_bytes(n)
        jobs.append((dev(w_np), dev(u_np), m, torch.empty(n, dtype=torch.uint8, device="cuda"),
                     torch.empty(nb, dtype=torch.uint8, device="cuda"), nb, heap_select(R, keys, m)))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for (w, u, m, flags, ws, nb, _), st in zip(jobs, streams):  # both enqueued before either is waited for
        assert _raw_call(L, w, u, m, flags, ws, nb, st.cuda_stream) == 0
    torch.cuda.synchronize()
    for w, u, m, flags, ws, nb, ref in jobs:
        assert np.array_equal(flags.cpu().numpy(), ref)


def test_sampling_kernels_do_not_spill():
    path = os.path.join(ROOT, "sycl_points_amd", "lib", "sampling.resources.txt")
    with open(path) as f:
        rows = [r for r in f.read().splitlines() if "sample_" in r or "weight_" in r]
    assert len(rows) >= 10, rows
    for r in rows:
        assert re.search(r"VGPRs Spill: 0\b", r) and re.search(r"ScratchSize \[bytes/lane\]: 0\b", r), r


def test_cpp_facade(sp):
    """tests/cpp/test_sampling.cpp, built with tests/cpp/Makefile's flags and libraries (the Makefile is not changed)."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(cpp, "test_sampling")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    lib = os.path.join(ROOT, "sycl_points_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++20", f"-I{ROOT}/include", f"-I{rocm}/include",
                           "-D__HIP_PLATFORM_AMD__", "-Wall", "-Wno-unused-value", "-Wno-unused-result",
                           os.path.join(cpp, "test_sampling.cpp"), "-o", exe, f"-L{lib}", "-lsycl_points_amd", f"-Wl,-rpath,{lib}",
                           f"-L{rocm}/lib", "-lamdhip64", f"-Wl,-rpath,{rocm}/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
