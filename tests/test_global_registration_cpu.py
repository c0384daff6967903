"""Global registration (csrc/global_registration.hip) without a GPU: the symbols, the triplet generator and sp_ransac_select_host
against the float64 model (tests/f64_fpfh.py), the argument errors that need no device, the compiler's resource report of the
unit, and the condition the GPU end-to-end test rests on: the model alone, on the bundled pair with the source turned by 150
degrees, puts a pose near the truth among its 64 best hypotheses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import f64_fpfh as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ("sp_fpfh_workspace_bytes", "sp_fpfh_compute", "sp_feature_match_workspace_bytes", "sp_feature_match",
           "sp_feature_match_mutual_workspace_bytes", "sp_feature_match_mutual", "sp_correspondence_points", "sp_ransac_score",
           "sp_ransac_triplets_host", "sp_ransac_select_host")
MAX_ROWS = 1 << 20  # SP_FEATURE_MATCH_MAX, SP_RANSAC_MAX_HYPOTHESES


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_symbols_and_abi(L):
    from sycl_points_amd import _lib

    for s in SYMBOLS:
        assert hasattr(L, s) and s in _lib.SIGNATURES, s
    assert L.sp_abi_version() == 7
    import sycl_points_amd.api as sp

    for name in ("fpfh", "match_features", "match_features_mutual", "ransac_scores", "ransac_select", "GlobalRegistrationParams"):
        assert hasattr(sp, name), name
    assert hasattr(sp.Registration, "align_global")
    p = sp.GlobalRegistrationParams()
    assert (p.hypotheses, p.guesses, p.edge_ratio) == (50000, 64, 0.9)


@pytest.mark.parametrize("seed,m", [(0, 3), (12345, 129), (2 ** 64 - 5, 465), (0x9E3779B97F4A7C15, (1 << 31) - 1)])
def test_triplet_generator_is_the_models(L, seed, m):
    got = np.zeros((1000, 3), np.uint32)
    assert L.sp_ransac_triplets_host(seed, 0, 1000, m, vp(got)) == 0
    want = model.triplets(seed, 1000, m)
    assert np.array_equal(got.astype(np.int64), want)
    assert want.max() < m and (m < 100 or len(np.unique(want)) > 50)
    late = np.zeros((7, 3), np.uint32)  # a window that does not start at 0
    assert L.sp_ransac_triplets_host(seed, (1 << 20) - 7, 7, m, vp(late)) == 0
    assert np.array_equal(late.astype(np.int64), model.triplets(seed, 7, m, first=(1 << 20) - 7))


def test_splitmix64_known_values():
    # the published test vector of splitmix64 seeded with 1234567: its first outputs
    z = np.uint64(1234567)
    out = []
    for _ in range(3):
        out.append(int(model.splitmix64(z)))
        with np.errstate(over="ignore"):
            z = z + np.uint64(0x9E3779B97F4A7C15)
    assert out == [6457827717110365317, 3203168211198807973, 9817491932198370423]


def select_host(L, scores, cs, ct, seed, guesses):
    scores = np.ascontiguousarray(scores, np.uint32)
    cs, ct = np.ascontiguousarray(cs, np.float32), np.ascontiguousarray(ct, np.float32)
    poses = np.full((max(guesses, 1), 16), np.nan)
    hyp = np.zeros(max(guesses, 1), np.uint32)
    count = C.c_size_t(99)
    rc = L.sp_ransac_select_host(vp(scores), len(scores), vp(cs), vp(ct), len(cs), seed, guesses, vp(poses), vp(hyp), C.byref(count))
    assert rc == 0
    v = int(count.value)
    return poses[:v].reshape(v, 4, 4).transpose(0, 2, 1), hyp[:v].astype(np.int64), poses


def congruent(m=40, seed=7):
    rs = np.random.RandomState(seed)
    cs = np.ones((m, 4), np.float32)
    cs[:, :3] = rs.uniform(-10, 10, (m, 3))
    a = rs.uniform(-1, 1, 3)
    a /= np.linalg.norm(a)
    th = 2.1
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    t = np.array([3.0, -2.0, 0.5])
    ct = np.ones((m, 4), np.float32)
    ct[:, :3] = cs[:, :3].astype(np.float64) @ R.T + t
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return cs, ct, T


def test_select_host_order_against_the_model(L):
    cs, ct, _ = congruent()
    seed = 11
    sc, _ = model.scores(cs, ct, 64, seed, 0.1, 0.5, 0.9)
    assert (sc > 0).sum() >= 8  # congruent triangles: every triplet that passes the gates explains every match
    hand = sc.copy()
    nz = np.nonzero(hand)[0]
    hand[nz[0]], hand[nz[3]], hand[nz[5]] = 7, 7, 9  # ties at 7 and at the common score, one hypothesis above
    for guesses in (1, 2, 5, len(nz), len(nz) + 10, 64, 1000):
        _, hyp, _ = select_host(L, hand, cs, ct, seed, guesses)
        want = model.select(hand, guesses)
        assert np.array_equal(hyp, want), (guesses, hyp, want)
        assert len(hyp) == min(guesses, len(nz))  # fewer nonzero scores than guesses: fewer poses
    _, hyp, raw = select_host(L, hand, cs, ct, seed, 0)  # B = 0: nothing written
    assert len(hyp) == 0 and np.isnan(raw).all()
    _, hyp, raw = select_host(L, np.zeros(64, np.uint32), cs, ct, seed, 8)  # no score
    assert len(hyp) == 0 and np.isnan(raw).all()
    _, hyp, _ = select_host(L, hand, cs[:2], ct[:2], seed, 8)  # fewer than three matches
    assert len(hyp) == 0


def test_select_host_poses_on_congruent_triangles(L):
    cs, ct, T = congruent()
    seed = 5
    sc, _ = model.scores(cs, ct, 256, seed, 0.1, 0.5, 0.9)
    poses, hyp, _ = select_host(L, sc, cs, ct, seed, 32)
    assert len(hyp) == 32
    want = model.poses(cs, ct, seed, hyp)
    assert np.abs(poses - want).max() <= 1e-12, np.abs(poses - want).max()
    assert np.array_equal(poses[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (32, 1)))
    assert np.abs(poses - T).max() < 1e-4  # the float32 rounding of the target points, through a triangle of edges > 0.5


def test_argument_errors_need_no_device(L):
    from sycl_points_amd import _lib

    bad = _lib.SP_ERR_INVALID_ARGUMENT
    p = C.c_void_p(4096)
    big = 1 << 40
    # sp_fpfh_compute(points, normals, n, idx, d2, k, out, counts, m, ws, ws_bytes, stream)
    assert L.sp_fpfh_compute(p, p, 100, p, p, 65, p, None, None, p, big, None) == bad and b"SP_FPFH_MAX_K" in L.sp_last_error()
    assert L.sp_fpfh_compute(p, p, 100, p, p, 0, p, None, None, p, big, None) == bad
    for hole in range(6):
        a = [p, p, p, p, p, p]
        a[hole] = None
        assert L.sp_fpfh_compute(a[0], a[1], 100, a[2], a[3], 20, a[4], None, None, a[5], big, None) == bad, hole
        assert b"null argument" in L.sp_last_error()
    need = L.sp_fpfh_workspace_bytes(100)
    assert need >= 100 * 36 * 4
    assert L.sp_fpfh_compute(p, p, 100, p, p, 20, p, None, None, p, need - 1, None) == bad and b"workspace" in L.sp_last_error()
    assert L.sp_fpfh_compute(p, p, 1 << 31, p, p, 20, p, None, None, p, big, None) == bad
    assert L.sp_fpfh_compute(None, None, 0, None, None, 20, None, None, None, None, 0, None) == 0  # n == 0: nothing to do
    # sp_feature_match(a, na, b, nb, idx, d2, ws, ws_bytes, stream)
    assert L.sp_feature_match_workspace_bytes(MAX_ROWS + 1, 10) == 0 and L.sp_feature_match_workspace_bytes(10, MAX_ROWS + 1) == 0
    assert L.sp_feature_match(p, MAX_ROWS + 1, p, 10, p, p, p, big, None) == bad and b"SP_FEATURE_MATCH_MAX" in L.sp_last_error()
    assert L.sp_feature_match(p, 10, p, MAX_ROWS + 1, p, p, p, big, None) == bad
    for hole in range(4):
        a = [p, p, p, p]
        a[hole] = None
        assert L.sp_feature_match(a[0], 10, a[1], 10, a[2], p, a[3], big, None) == bad, hole
    need = L.sp_feature_match_workspace_bytes(100, 50)
    assert need >= 8 * 100 + 4 * 150
    assert L.sp_feature_match(p, 100, p, 50, p, p, p, need - 1, None) == bad and b"workspace" in L.sp_last_error()
    assert L.sp_feature_match(C.c_void_p(4100), 100, p, 50, p, p, p, big, None) == bad and b"aligned" in L.sp_last_error()
    # sp_feature_match_mutual(src, ns, tgt, nt, corr, count, ws, ws_bytes, stream)
    cnt = C.c_uint32(5)
    assert L.sp_feature_match_mutual(p, MAX_ROWS + 1, p, 10, p, C.byref(cnt), p, big, None) == bad
    assert L.sp_feature_match_mutual(p, 10, p, 10, p, None, p, big, None) == bad
    assert L.sp_feature_match_mutual(p, 10, p, 10, None, C.byref(cnt), p, big, None) == bad
    need = L.sp_feature_match_mutual_workspace_bytes(100, 50)
    assert need > L.sp_feature_match_workspace_bytes(100, 50)
    assert L.sp_feature_match_mutual(p, 100, p, 50, p, C.byref(cnt), p, need - 1, None) == bad
    assert L.sp_feature_match_mutual(p, 0, p, 50, p, C.byref(cnt), p, big, None) == 0 and cnt.value == 0  # an empty side: no pair
    # sp_ransac_score(cs, ct, m, H, seed, tau, min_edge, ratio, score, stream)
    assert L.sp_ransac_score(p, p, 100, MAX_ROWS + 1, 0, 1.0, 0.0, 0.9, p, None) == bad
    assert L.sp_ransac_score(p, p, 100, 64, 0, 1.0, 0.0, 0.9, None, None) == bad
    assert L.sp_ransac_score(None, p, 100, 64, 0, 1.0, 0.0, 0.9, p, None) == bad
    assert L.sp_ransac_score(p, p, 100, 64, 0, -1.0, 0.0, 0.9, p, None) == bad
    assert L.sp_ransac_score(p, p, 100, 64, 0, 1.0, 0.0, 1.5, p, None) == bad
    # sp_ransac_select_host / sp_ransac_triplets_host
    n = C.c_size_t(3)
    assert L.sp_ransac_select_host(None, 10, None, None, 10, 0, 4, None, None, C.byref(n)) == bad and n.value == 0
    assert L.sp_ransac_select_host(None, MAX_ROWS + 1, None, None, 10, 0, 4, None, None, C.byref(n)) == bad
    assert L.sp_ransac_triplets_host(0, 0, 4, 10, None) == bad
    # sp_correspondence_points
    assert L.sp_correspondence_points(None, 5, p, 5, p, 3, p, p, None) == bad
    assert L.sp_correspondence_points(p, 0, p, 5, p, 3, p, p, None) == bad


def test_no_kernel_of_the_unit_uses_scratch(L):
    rows = [l for l in open(os.path.join(ROOT, "sycl_points_amd", "lib", "global_registration.resources.txt")) if "Function Name" in l]
    names = " ".join(rows)
    for kernel in ("spfh_kernel", "fpfh_kernel", "match_kernel", "ransac_score_kernel", "norms_kernel", "mutual_flags_kernel"):
        assert kernel in names, kernel
    for row in rows:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", row).group(1)) == 0, row
        assert int(re.search(r"VGPRs Spill: (\d+)", row).group(1)) == 0, row


def test_the_model_relocalises_the_bundled_pair():
    """1 m voxels, k = 20, 50 000 hypotheses, tau = 1 m: at least one of the 64 best hypotheses lies within 0.1 rad / 1 m of the
    truth (the feasibility check had 60 of 64)."""
    clouds, T_true = model.bundled_pair(GOLD, voxel=1.0, k=20)
    (sx, sn, si, sd), (tx, tn, ti, td) = clouds["source"], clouds["target"]
    fs, ft = model.fpfh(sx, sn, si, sd), model.fpfh(tx, tn, ti, td)
    corr = model.mutual(fs, ft)
    cs, ct = sx[corr[:, 0]], tx[corr[:, 1]]
    moved = cs @ T_true[:3, :3].T + T_true[:3, 3]
    good = int((np.linalg.norm(moved - ct, axis=1) < 1.0).sum())
    seed = 2024
    sc, _ = model.scores(cs, ct, 50000, seed, 1.0, 0.0, 0.9)
    best = model.select(sc, 64)
    errs = [model.pose_errors(T, T_true) for T in model.poses(cs, ct, seed, best)]
    near = sum(1 for dt, dr in errs if dt <= 1.0 and dr <= 0.1)
    print(f"\n[global registration, model] {len(sx)} / {len(tx)} points, {len(corr)} mutual matches, {good} within 1 m of the truth, "
          f"{len(best)} hypotheses kept, {near} within 0.1 rad / 1 m")
    assert len(best) == 64 and near >= 1
