"""Compatibility-graph guesses (csrc/correspondence_graph.hip) without a GPU: the symbols, the host twins of
steps 1-4 against the model of tests/f64_compat.py bit for bit (degrees, second-order sums, seed order, consensus lists) at
M = 3, 4, 31, 32, 33, 65, 200 and on engineered boundaries, the host poses against the model's SVD, the selection, the argument
errors that need no device, and the compiler's resource report of the unit.

The pose bound: both sides are double; Horn's quaternion form by Jacobi rotations on one side, Kabsch by LAPACK's SVD on the
other. Entries of T are <= 70 (a 60 x 40 x 6 m hall, 5 m of translation): 1e-9 absolute is 1.4e-11 relative, five orders above
the rounding of either solver on sets whose scatter matrices have a condition number below 1e4."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import f64_compat as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sp_compat_workspace_bytes", "sp_compat_seeds", "sp_compat_consensus", "sp_compat_seeds_host", "sp_compat_consensus_host",
           "sp_compat_poses_host", "sp_pose_score", "sp_compat_select_host")
F = np.float32


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_seeds(L, cs, ct, tau, min_edge, seeds):
    cs, ct = np.ascontiguousarray(cs, F), np.ascontiguousarray(ct, F)
    m = len(cs)
    idx, sv = np.full(max(seeds, 1), 7, np.int32), np.full(max(seeds, 1), 7, np.uint32)
    deg, s = np.full(max(m, 1), 7, np.uint32), np.full(max(m, 1), 7, np.uint32)
    assert L.sp_compat_seeds_host(vp(cs), vp(ct), m, tau, min_edge, seeds, vp(idx), vp(sv), vp(deg), vp(s)) == 0
    return idx[:seeds], sv[:seeds], deg[:m].astype(np.int64), s[:m].astype(np.int64)


def host_lists(L, cs, ct, tau, min_edge, seed_idx, k):
    cs, ct = np.ascontiguousarray(cs, F), np.ascontiguousarray(ct, F)
    seed_idx = np.ascontiguousarray(seed_idx, np.int32)
    n = len(seed_idx)
    cons, cons_s = np.full((max(n, 1), k), 7, np.int32), np.full((max(n, 1), k), 7, np.uint32)
    assert L.sp_compat_consensus_host(vp(cs), vp(ct), len(cs), tau, min_edge, vp(seed_idx), n, k, vp(cons), vp(cons_s)) == 0
    return cons[:n], cons_s[:n]


def host_poses(L, cs, ct, seed_idx, cons):
    cs, ct = np.ascontiguousarray(cs, F), np.ascontiguousarray(ct, F)
    seed_idx, cons = np.ascontiguousarray(seed_idx, np.int32), np.ascontiguousarray(cons, np.int32)
    n, k = cons.shape
    poses, rank, count = np.zeros((max(n, 1), 16)), np.zeros(max(n, 1), np.uint32), C.c_size_t(99)
    assert L.sp_compat_poses_host(vp(cs), vp(ct), len(cs), vp(seed_idx), vp(cons), n, k, vp(poses), vp(rank), C.byref(count)) == 0
    v = int(count.value)
    return poses[:v].reshape(v, 4, 4).transpose(0, 2, 1), rank[:v].astype(np.int64)


def padded(lists, n, k):
    out = np.full((n, k), -1, np.int32)
    for r, row in enumerate(lists):
        out[r, :len(row)] = row
    return out


def check_against_model(L, cs, ct, tau, min_edge, seeds, k, tag):
    """degrees, s, seeds and lists of the host twins are the model's; returns the model's (seed_idx, lists)"""
    deg, s, seed_idx, lists = model.seeds_and_lists(cs, ct, tau, min_edge, seeds, k)
    idx, sv, hdeg, hs = host_seeds(L, cs, ct, tau, min_edge, seeds)
    print(f"\n[compat host {tag}] M {len(cs)}: {int(deg.sum()) // 2} edges, max s {int(s.max()) if len(s) else 0}, {len(seed_idx)} seeds", end="")
    assert np.array_equal(hdeg, deg), np.flatnonzero(hdeg != deg)[:5]
    assert np.array_equal(hs, s), np.flatnonzero(hs != s)[:5]
    want_idx = np.full(seeds, -1, np.int32)
    want_idx[:len(seed_idx)] = seed_idx
    assert np.array_equal(idx, want_idx), (idx, want_idx)
    assert np.array_equal(sv[:len(seed_idx)].astype(np.int64), s[seed_idx]) and not sv[len(seed_idx):].any()
    cons, cons_s = host_lists(L, cs, ct, tau, min_edge, idx, k)
    assert np.array_equal(cons, padded(lists, seeds, k)), (cons, lists)
    assert ((cons_s > 0) == (cons >= 0)).all()
    return seed_idx, lists


# ------------------------------------------------------------------------------------------------------------------ symbols
def test_symbols_and_abi(L):
    from sycl_points_amd import _lib

    for s in SYMBOLS:
        assert hasattr(L, s) and s in _lib.SIGNATURES, s
    assert L.sp_abi_version() == 7
    assert (_lib.COMPAT_MAX_MATCHES, _lib.COMPAT_MAX_SEEDS, _lib.COMPAT_MAX_K) == (8192, 256, 64)
    assert L.sp_compat_workspace_bytes(8193) == 0
    assert L.sp_compat_workspace_bytes(200) == 256 * 256 + 1036 * 256 and L.sp_compat_workspace_bytes(8192) == 8192 * 8192 + 1036 * 8192
    header = open(os.path.join(ROOT, "include", "sycl_points_amd.h")).read()
    assert "SP_COMPAT_MAX_MATCHES = 8192, SP_COMPAT_MAX_SEEDS = 256, SP_COMPAT_MAX_K = 64" in header
    import sycl_points_amd.api as sp

    for name in ("compat_seeds", "compat_consensus", "pose_scores", "compat_guesses", "compat_poses", "compat_select"):
        assert hasattr(sp, name), name
    p = sp.GlobalRegistrationParams()
    assert (p.method, p.compat_tau, p.compat_seeds, p.compat_k) == ("TRIPLETS", 0.1, 64, 16)
    assert (p.hypotheses, p.guesses, p.inlier_distance, p.min_edge, p.edge_ratio, p.seed) == (50000, 64, 1.0, 0.0, 0.9, 0)


# --------------------------------------------------------------------------------------------------------- steps 1-4, shapes
@pytest.mark.parametrize("m", [3, 4, 31, 32, 33, 65, 200])
def test_host_twins_are_the_models(L, m):
    cs, ct, _, mask = model.hall_matches(m, max(3, m // 4), 100 + m)
    seed_idx, lists = check_against_model(L, cs, ct, 0.1, 1.0, 64, 16, f"hall {m}")
    assert len(seed_idx) >= 3 and mask[seed_idx[0]]  # the check is not vacuous: the best seed is an inlier
    check_against_model(L, cs, ct, 0.25, 0.0, 5, 3, f"hall {m}, 5 seeds of 3")


# ----------------------------------------------------------------------------------------------------- engineered boundaries
def rows(xyz):
    out = np.ones((len(xyz), 4), F)
    out[:, :3] = np.asarray(xyz, F)
    return out


def triangle_fan():
    """a rigid cluster every special match below is attached to: 6 matches under the identity, pairwise more than 1 apart"""
    return [(10, 0, 0), (10, 4, 0), (13, 0, 2), (13, 4, 2), (16, 1, 0), (16, 5, 3)]


TAU_LENGTHS = [F(2.5), np.nextafter(F(2.5), F(0)), np.nextafter(F(2.5), F(3)), F(1.5), np.nextafter(F(1.5), F(0)), np.nextafter(F(1.5), F(3)),
               F(2.5 * (1 - 1e-6)), F(1.5 * (1 + 1e-6))]


def tau_boundary_case():
    """source pairs of length 2 along x against target pairs of the lengths above, each pair 100 away from the next, plus the fan"""
    src, tgt = list(triangle_fan()), list(triangle_fan())
    for i, g in enumerate(TAU_LENGTHS):  # pair i: matches (6 + 2 i, 7 + 2 i)
        y = 100.0 * (i + 1)
        src += [(0, y, 0), (2, y, 0)]
        tgt += [(0, y, 0), (float(g), y, 0)]
    return rows(src), rows(tgt)


def test_length_difference_exactly_tau_and_one_ulp_either_side(L):
    """source pairs of length 2 against target pairs of length 2.5 and 1.5, their float32 neighbours on either side, and lengths a
    relative 1e-6 (16 ulp) inside: tau = 0.5 met exactly gives q^2 == 4 u v == 100 and 36 == 36, not compatible (the test is
    strict); one ulp of the coordinate either side is below what the float32 expression resolves, so there the model decides and
    the twins follow it bit for bit; 16 ulp inside is compatible."""
    tau = 0.5
    cs, ct = tau_boundary_case()
    Cm = model.compatibility(cs, ct, tau, 0.0)
    got = [int(Cm[6 + 2 * i, 7 + 2 * i]) for i in range(len(TAU_LENGTHS))]
    print(f"\n[compat boundary tau] C of the pairs (exactly +tau, one ulp inside, outside, exactly -tau, one ulp outside, inside, "
          f"16 ulp inside +tau, 16 ulp inside -tau): {got}", end="")
    assert got[0] == 0 and got[3] == 0 and got[2] == 0 and got[4] == 0 and got[6] == 1 and got[7] == 1
    assert np.array_equal(Cm, Cm.T)
    check_against_model(L, cs, ct, tau, 0.0, 64, 16, "tau boundary")


def min_edge_case():
    src = list(triangle_fan()) + [(10, 1, 0), (10, float(np.nextafter(F(1), F(2))), 0), (10, 0, 1), (11, 0, 0)]
    return rows(src), rows(src)


def test_edges_exactly_at_min_edge(L):
    """min_edge = 1: an edge of length exactly 1 is not longer than min_edge; one ulp more is"""
    cs, ct = min_edge_case()
    Cm = model.compatibility(cs, ct, 0.1, 1.0)
    assert Cm[0, 6] == 0 and Cm[0, 7] == 1 and Cm[0, 8] == 0 and Cm[0, 9] == 0  # (10, 0, 0) against its four neighbours
    check_against_model(L, cs, ct, 0.1, 1.0, 64, 16, "min_edge boundary")
    check_against_model(L, cs, ct, 0.1, 0.0, 64, 16, "min_edge 0")


def duplicates_case():
    cs, ct, _, _ = model.hall_matches(40, 12, 7)
    cs[5], ct[5] = cs[3], ct[3]          # the same match twice: never compatible with its twin (u == 0)
    cs[9] = cs[8]                        # the same source point with two targets
    ct[20] = ct[21]
    return cs, ct


def all_outliers_case():
    rs = np.random.RandomState(3)
    return rows(rs.uniform(0, 50, (33, 3))), rows(np.tile([[1.0, 2.0, 3.0]], (33, 1)))  # every target edge has length 0


def test_duplicate_points(L):
    cs, ct = duplicates_case()
    Cm = model.compatibility(cs, ct, 0.1, 0.0)
    assert Cm[5, 3] == 0 and Cm[9, 8] == 0 and Cm[20, 21] == 0
    check_against_model(L, cs, ct, 0.1, 0.0, 64, 16, "duplicates")


def test_all_outliers_give_nothing(L):
    cs, ct = all_outliers_case()
    seed_idx, lists = check_against_model(L, cs, ct, 0.1, 0.0, 64, 16, "all outliers")
    assert seed_idx == [] and lists == []
    idx, sv, deg, s = host_seeds(L, cs, ct, 0.1, 0.0, 64)
    assert (idx == -1).all() and not sv.any() and not deg.any() and not s.any()
    cons, _ = host_lists(L, cs, ct, 0.1, 0.0, idx, 16)
    assert (cons == -1).all()
    poses, rank = host_poses(L, cs, ct, idx, cons)
    assert len(poses) == 0


def two_cliques():
    """two rigid clusters of 5 under different motions, far apart: no edge between them"""
    a = np.array([(0, 0, 0), (3, 0, 0), (0, 4, 0), (0, 0, 5), (3, 4, 1)], np.float64)
    b = a[:, [1, 2, 0]] * 1.5 + [200.0, 0.0, 0.0]
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    cs = rows(np.r_[a, b])
    ct = rows(np.r_[a + [1.0, 2.0, 3.0], b @ Rz.T + [0.0, 500.0, 7.0]])
    return cs, ct


def test_two_equal_cliques_tie_to_the_lower_index(L):
    cs, ct = two_cliques()
    Cm = model.compatibility(cs, ct, 0.05, 0.0)
    assert Cm[:5, :5].sum() == 20 and Cm[5:, 5:].sum() == 20 and Cm[:5, 5:].sum() == 0
    seed_idx, lists = check_against_model(L, cs, ct, 0.05, 0.0, 64, 16, "two cliques")
    assert seed_idx == list(range(10))  # s = 4 x 3 = 12 everywhere: index order
    assert lists[0] == [1, 2, 3, 4] and lists[7] == [5, 6, 8, 9]
    idx, sv, _, _ = host_seeds(L, cs, ct, 0.05, 0.0, 3)  # fewer seeds than ties
    assert list(idx) == [0, 1, 2] and list(sv) == [12, 12, 12]
    cons, cons_s = host_lists(L, cs, ct, 0.05, 0.0, [7, -1, 0], 2)  # fewer companions than ties; an empty slot in the middle
    assert cons.tolist() == [[5, 6], [-1, -1], [1, 2]] and cons_s.tolist() == [[3, 3], [0, 0], [3, 3]]


# -------------------------------------------------------------------------------------------------------------------- poses
def test_host_poses_are_the_models_svd(L):
    cs, ct, T_true, mask = model.hall_matches(200, 50, 300)
    seed_idx, lists = check_against_model(L, cs, ct, 0.1, 1.0, 64, 16, "hall 200 for poses")
    want, want_rank = model.poses(cs, ct, seed_idx, lists)
    idx = np.full(64, -1, np.int32)
    idx[:len(seed_idx)] = seed_idx
    got, rank = host_poses(L, cs, ct, idx, padded(lists, 64, 16))
    err = float(np.abs(got - want).max())
    et, er = model.pose_errors(got[0], T_true)
    print(f" | {len(got)} poses, max |T_host - T_svd| {err:.2e}, first pose {et:.3f} m / {er:.4f} from the truth")
    assert len(got) == len(want) >= 30 and np.array_equal(rank, want_rank)
    assert err <= 1e-9
    assert np.abs(got[:, 3] - [0, 0, 0, 1]).max() == 0
    assert max(abs(np.linalg.det(T[:3, :3]) - 1.0) for T in got) < 1e-12


def test_degenerate_sets_yield_no_pose(L):
    """a seed with exactly one companion is dropped; so is a collinear set; a planar set (rank 2) is kept"""
    line = [(float(i), 2.0 * i, -1.0 * i) for i in range(6)]
    plane = [(0, 0, 0), (4, 0, 0), (0, 3, 0), (4, 3, 0), (1, 1, 0), (2, 5, 0)]
    cs = rows(line + plane)
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    ct = rows(np.asarray(line + plane, np.float64) @ Rz.T + [1.0, 2.0, 3.0])
    seed_idx = [0, 6, 7, 1, -1]
    lists = [[1, 2, 3, 4, 5], [7], [6, 8, 9, 10, 11], [2, 7], []]  # collinear; one companion; planar; general; empty slot
    got, rank = host_poses(L, cs, ct, seed_idx, padded(lists, 5, 5))
    want, want_rank = model.poses(cs, ct, seed_idx[:4], lists[:4])
    assert list(rank) == [2, 3] == list(want_rank)
    assert np.abs(got - want).max() <= 1e-9
    assert np.abs(got[0][:3, :3] - Rz).max() < 1e-12 and np.abs(got[0][:3, 3] - [1, 2, 3]).max() < 1e-12
    # k < 2: no set can have two companions
    got, rank = host_poses(L, cs, ct, [6], padded([[7]], 1, 1))
    assert len(got) == 0


def test_select_takes_the_best_scores_and_earlier_ranks_first(L):
    scores = np.array([5, 9, 0, 9, 7, 5], np.uint32)
    poses = np.arange(6 * 16, dtype=np.float64).reshape(6, 16)
    ranks = np.array([0, 2, 3, 5, 8, 9], np.uint32)
    out, out_rank, count = np.zeros((4, 16)), np.zeros(4, np.uint32), C.c_size_t(0)
    assert L.sp_compat_select_host(vp(scores), vp(poses), vp(ranks), 6, 4, vp(out), vp(out_rank), C.byref(count)) == 0
    assert count.value == 4 and list(out_rank) == [2, 5, 8, 0] and np.array_equal(out, poses[[1, 3, 4, 0]])
    assert L.sp_compat_select_host(vp(scores), vp(poses), None, 6, 4, vp(out), vp(out_rank), C.byref(count)) == 0
    assert list(out_rank) == [1, 3, 4, 0]
    big = np.zeros((8, 16))
    assert L.sp_compat_select_host(vp(scores), vp(poses), vp(ranks), 6, 8, vp(big), None, C.byref(count)) == 0
    assert count.value == 5  # the zero score is never a guess
    assert L.sp_compat_select_host(vp(np.zeros(6, np.uint32)), vp(poses), vp(ranks), 6, 8, vp(big), None, C.byref(count)) == 0 and count.value == 0


def test_model_guesses_on_the_hall(L):
    """steps 1-7 of the model on 5 % inliers: every guess near the truth; the scores the model counts are the host pipeline's"""
    cs, ct, T_true, mask = model.hall_matches(400, 20, 11)
    T, ranks, sc = model.guesses(cs, ct, 0.1, 1.0, 64, 16, 0.3, 8)
    et, er = model.pose_errors(T[0], T_true)
    print(f"\n[compat model] 20 of 400: best guess explains {int(sc[0])}, {et:.3f} m / {er:.4f} from the truth")
    assert sc[0] >= 18 and et < 0.05 and er < 0.005


# --------------------------------------------------------------------------------------------------------------- arguments
def test_argument_errors_need_no_device(L):
    cs, ct, _, _ = model.hall_matches(8, 4, 1)
    idx, sv = np.zeros(256, np.int32), np.zeros(256, np.uint32)
    ws = np.zeros(1 << 20, np.uint8)
    need = L.sp_compat_workspace_bytes(8)
    assert 0 < need <= ws.nbytes and ws.ctypes.data % 16 == 0
    bad = 1  # SP_ERR_INVALID_ARGUMENT

    def seeds(m=8, tau=0.1, min_edge=0.0, n=4, a=cs, b=ct, i=idx, s=sv, w=ws, wb=None):
        return L.sp_compat_seeds(vp(a), vp(b), m, tau, min_edge, n, vp(i), vp(s), None, None, vp(w), need if wb is None else wb, None)

    assert seeds(m=8193) == bad and b"SP_COMPAT_MAX_MATCHES" in L.sp_last_error()
    assert seeds(n=257) == bad and seeds(tau=0.0) == bad and seeds(tau=float("nan")) == bad and seeds(min_edge=-1.0) == bad
    assert seeds(a=None) == bad and seeds(b=None) == bad and seeds(i=None) == bad and seeds(s=None) == bad and seeds(w=None) == bad
    assert seeds(wb=need - 1) == bad and b"workspace" in L.sp_last_error()

    cons = np.zeros((4, 16), np.int32)

    def consensus(m=8, n=4, k=16, i=idx, c=cons, w=ws, wb=None):
        return L.sp_compat_consensus(m, vp(i), n, k, vp(c), None, vp(w), need if wb is None else wb, None)

    assert consensus(m=8193) == bad and consensus(n=257) == bad and consensus(k=65) == bad
    assert consensus(i=None) == bad and consensus(c=None) == bad and consensus(w=None) == bad and consensus(wb=16) == bad
    assert consensus(n=0) == 0 and consensus(k=0) == 0  # nothing to do: no HIP call either

    score = np.zeros(4, np.uint32)
    poses = np.zeros((4, 16), F)
    assert L.sp_pose_score(vp(cs), vp(ct), 8, vp(poses), (1 << 20) + 1, 1.0, vp(score), None) == bad
    assert L.sp_pose_score(vp(cs), vp(ct), 8, None, 4, 1.0, vp(score), None) == bad
    assert L.sp_pose_score(vp(cs), vp(ct), 8, vp(poses), 4, 1.0, None, None) == bad
    assert L.sp_pose_score(None, vp(ct), 8, vp(poses), 4, 1.0, vp(score), None) == bad
    assert L.sp_pose_score(vp(cs), vp(ct), 8, vp(poses), 4, -1.0, vp(score), None) == bad
    assert L.sp_pose_score(vp(cs), vp(ct), 8, vp(poses), 0, 1.0, vp(score), None) == 0

    # the host twins: the same limits; M < 3 gives empty lists
    deg, s = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
    assert L.sp_compat_seeds_host(vp(cs), vp(ct), 8193, 0.1, 0.0, 4, vp(idx), vp(sv), None, None) == bad
    assert L.sp_compat_seeds_host(vp(cs), vp(ct), 8, 0.1, 0.0, 257, vp(idx), vp(sv), None, None) == bad
    assert L.sp_compat_seeds_host(vp(cs), vp(ct), 8, -0.1, 0.0, 4, vp(idx), vp(sv), None, None) == bad
    assert L.sp_compat_seeds_host(None, vp(ct), 8, 0.1, 0.0, 4, vp(idx), vp(sv), None, None) == bad
    assert L.sp_compat_seeds_host(vp(cs), vp(ct), 8, 0.1, 0.0, 4, None, vp(sv), None, None) == bad
    for m in (0, 1, 2):
        idx[:], sv[:] = 7, 7
        assert L.sp_compat_seeds_host(vp(cs), vp(ct), m, 0.1, 0.0, 4, vp(idx), vp(sv), vp(deg), vp(s)) == 0
        assert (idx[:4] == -1).all() and not sv[:4].any() and idx[4] == 7
        cons[:] = 7
        assert L.sp_compat_consensus_host(vp(cs), vp(ct), m, 0.1, 0.0, vp(idx), 4, 16, vp(cons), None) == 0 and (cons == -1).all()
    assert L.sp_compat_consensus_host(vp(cs), vp(ct), 8, 0.1, 0.0, vp(idx), 4, 65, vp(cons), None) == bad
    count = C.c_size_t(5)
    out = np.zeros((4, 16))
    assert L.sp_compat_poses_host(vp(cs), vp(ct), 8, vp(idx), vp(cons), 4, 65, vp(out), None, C.byref(count)) == bad and count.value == 0
    assert L.sp_compat_poses_host(vp(cs), vp(ct), 8, vp(idx), vp(cons), 4, 16, vp(out), None, None) == bad
    assert L.sp_compat_poses_host(vp(cs), vp(ct), 8, None, vp(cons), 4, 16, vp(out), None, C.byref(count)) == bad
    assert L.sp_compat_poses_host(vp(cs), vp(ct), 2, vp(idx), vp(cons), 4, 16, vp(out), None, C.byref(count)) == 0 and count.value == 0
    assert L.sp_compat_select_host(None, vp(out), None, 4, 4, vp(out), None, C.byref(count)) == bad
    assert L.sp_compat_select_host(vp(score), vp(out), None, 4, 4, vp(out), None, None) == bad


# ------------------------------------------------------------------------------------------------------- the resource report
def test_resource_report_has_no_scratch_and_no_spills(L):
    rows_ = [l for l in open(os.path.join(ROOT, "sycl_points_amd", "lib", "correspondence_graph.resources.txt")) if "Function Name" in l]
    names = " ".join(rows_)
    for kernel in ("compat_kernel", "second_order_kernel", "seed_rank_kernel", "seed_scatter_kernel", "seed_rows_kernel", "consensus_kernel", "pose_score_kernel"):
        assert kernel in names, kernel
    for row in rows_:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", row).group(1)) == 0, row
        assert int(re.search(r"VGPRs Spill: (\d+)", row).group(1)) == 0, row
