"""The reference-topology KD-tree on the device (csrc/kdtree.hip: what KDTree.build(points) gives, and what the accelerated
tree falls back to for k > 32, below 1024 points and for the reference's tie order) and the seam that chooses a structure per
call (csrc/knn_tree.hip), at every list class of dispatch_search and its edges, every leaf loop, both radius modes, every
transform mode, the 200 000-query switch, the far stack when it overflows, lazy deletes and non-finite queries.

Every row is compared with two things (tests/f64_knn.py): the oracle's KD-tree bit for bit — indices and distances; this pins
the traversal order, the first-visited tie rule and the far-stack drop — and a float64 brute force written in the test
helper, independent of the oracle (range, order, padding, |d - D| <= 6 u D, completeness within 12 u, the entry count of a
radius search). tests/test_oracle_kdtree_f64.py holds the oracle to the same yardstick on the same clouds.

kdtree_search_kernel<KCAP, RADIUS, BATCH_LEAF> instantiations by test:
  kernel matrix kNN      <1,F,F> <10,F,T> <20,F,T> <50,F,F> <100,F,F>   (k = 1 | 2, 10 | 11, 20 | 21, 50 | 51, 100)
  full leaf blocks       the same five, and <1,T,F> <10,T,T> <100,T,F>, on trees whose every leaf slot holds a point
  kernel matrix radius   <1,T,F> <10,T,T> <20,T,T> <50,T,F> <100,T,F>
  many queries           <10,F,F> <20,F,F> <10,T,F> <20,T,F>            (200 704 queries)
  ties, far stack, lazy delete, non-finite, seam: <100,F,F> <50,F,F> <100,T,F> <50,T,F> <1,F,F> <10,F,T> again
"""
import ctypes as C

import numpy as np
import pytest

import f64_knn as Y
from test_gpu_bvh import nonuniform_cloud

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
FLT_MAX = Y.FLT_MAX
KS = (1, 2, 10, 11, 20, 21, 50, 51, 100)
RADII = (0.3, 1.0, 2.0, 4.0)  # at 5 points per unit volume: about 0.6, 21, 170 and 1300 points in the ball
TWIST = np.float32([0.05, -0.1, 0.02, 0.2, -0.1, 0.1])


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


@pytest.fixture(scope="module")
def cloud(orc):
    tgt, qry = Y.matrix_cloud(orc)
    D = Y.brute_d2(qry, tgt)
    return tgt, qry, D, Y.top_sorted(D, 100)


@pytest.fixture(scope="module")
def moved(orc, cloud):
    """The queries under a transform: T, the queries as they are searched (checked against float64) and their yardstick."""
    tgt, qry, _, _ = cloud
    T = orc.se3_exp(TWIST)
    qT = Y.transformed_f64_checked(qry, T, orc.transform_points(qry, T))
    D = Y.brute_d2(qT, tgt)
    return T, D, Y.top_sorted(D, 100)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pose_on_device(T):
    return dev(np.asarray(T, np.float32).T.reshape(16))  # column-major


def host(r):
    return r.indices.cpu().numpy(), r.distances.cpu().numpy()


def radius_search(tree, queries, max_k, radius, transT=None):
    from sycl_points_amd.api import KNNResult

    r = KNNResult()
    tree.radius_search_async(queries, max_k, radius, r, transT)
    return r


def same_rows(r, oi, od):
    gi, gd = host(r)
    assert np.array_equal(gd, od), "distances differ from the oracle's tree"
    assert np.array_equal(gi, oi), "indices differ from the oracle's tree"
    return gi, gd


@pytest.mark.parametrize("leaf", [1, 5, 16, 33])
def test_kernel_matrix_knn(sp, orc, cloud, leaf):
    tgt, qry, D, top = cloud
    fig = Y.Figures()
    tree = sp.KDTree.build(dev(tgt), leaf)
    nodes = orc.kdtree_build(tgt, leaf)
    Q = dev(qry)
    for k in KS:
        gi, gd = same_rows(tree.knn_search(Q, k), *orc.kdtree_knn(nodes, qry, k))
        Y.check_rows(gi, gd, D, top=top, figures=fig)
    print(f"device kNN, leaf {leaf}: {fig}")


def test_kernel_matrix_knn_root_leaf_block_and_padded_rows(sp, orc, cloud):
    tgt, qry, D, _ = cloud
    fig = Y.Figures()
    Q = dev(qry)
    small = tgt[:150]  # leaf 4096: the root is one leaf block of 150 slots in a stride of 4096
    tree = sp.KDTree.build(dev(small), 4096)
    nodes = orc.kdtree_build(small, 4096)
    for k in KS:
        gi, gd = same_rows(tree.knn_search(Q, k), *orc.kdtree_knn(nodes, qry, k))
        Y.check_rows(gi, gd, D[:, :150], figures=fig)
    for leaf in (1, 16, 33):  # 17 points, k = 100: 83 padded entries a row
        tree = sp.KDTree.build(dev(tgt[:17]), leaf)
        gi, gd = same_rows(tree.knn_search(Q, 100), *orc.kdtree_knn(orc.kdtree_build(tgt[:17], leaf), qry, 100))
        Y.check_rows(gi, gd, D[:, :17], figures=fig)
        assert ((gi >= 0).sum(1) == 17).all()
    print(f"device kNN, root leaf / padded: {fig}")


@pytest.mark.parametrize("leaf", [1, 5, 16, 33, 4096])
def test_kernel_matrix_leaf_blocks_without_a_pad_slot(sp, orc, cloud, leaf):
    """(leaf + 1) 2^m - 1 points: every median split is exact and every leaf block is full to its last slot. On the 5000-point
    cloud the blocks of leaf 5 hold three or four points and those of leaf 33 eighteen or nineteen — a leaf loop that stopped a
    slot early would pass there."""
    tgt, qry, D, _ = cloud
    n = Y.full_leaves_size(leaf)
    assert n == {1: 4095, 5: 3071, 16: 4351, 33: 4351, 4096: 4096}[leaf]
    full, D = tgt[:n], D[:, :n]
    top = Y.top_sorted(D, 100)
    fig = Y.Figures()
    tree = sp.KDTree.build(dev(full), leaf)
    nodes = orc.kdtree_build(full, leaf)
    leaves = np.frombuffer(nodes.tobytes(), np.int32).reshape(-1, 8)  # (oracle_knn.hpp FlatKDNode: idx, left, right = words 4..6)
    is_block = (np.frombuffer(nodes.tobytes(), np.uint8).reshape(-1, 32)[:, 29] == 1) & (leaves[:, 4] == -1)
    assert is_block.any() and (leaves[is_block, 6] == leaf).all()  # every leaf block holds `leaf` points
    Q = dev(qry)
    for k in KS:
        gi, gd = same_rows(tree.knn_search(Q, k), *orc.kdtree_knn(nodes, qry, k))
        Y.check_rows(gi, gd, D, top=top, figures=fig)
    for max_k in (1, 10, 100):
        gi, gd = same_rows(radius_search(tree, Q, max_k, 1.5), *orc.kdtree_radius(nodes, qry, max_k, 1.5))
        Y.check_rows(gi, gd, D, radius=1.5, top=top, figures=fig)
    for k in (1, 2, 21):  # every point as a query finds itself first: no slot of any block can be skipped unnoticed
        gi, gd = same_rows(tree.knn_search(dev(full), k), *orc.kdtree_knn(nodes, full, k))
        assert np.array_equal(gi[:, 0], np.arange(n)) and (gd[:, 0] == 0).all()
    print(f"device, full leaf blocks, leaf {leaf}: {fig}")


@pytest.mark.parametrize("leaf", [5, 16])
def test_kernel_matrix_radius(sp, orc, cloud, moved, leaf):
    tgt, qry, D, top = cloud
    T, DT, topT = moved
    fig = Y.Figures()
    tree = sp.KDTree.build(dev(tgt), leaf)
    nodes = orc.kdtree_build(tgt, leaf)
    Q, T_dev = dev(qry), pose_on_device(T)
    empty = short = full = ambiguous = 0
    for max_k in (1, 10, 20, 50, 100):
        for radius in RADII:
            oi, od = orc.kdtree_radius(nodes, qry, max_k, radius)
            gi, gd = same_rows(radius_search(tree, Q, max_k, radius), oi, od)
            ambiguous += Y.check_rows(gi, gd, D, radius=radius, top=top, figures=fig)
            n = (gi >= 0).sum(1)
            empty, short, full = empty + (n == 0).sum(), short + ((n > 0) & (n < max_k)).sum(), full + (n == max_k).sum()
            oi, od = orc.kdtree_radius(nodes, qry, max_k, radius, T)
            gi, gd = same_rows(radius_search(tree, Q, max_k, radius, T), oi, od)  # a host 4x4
            Y.check_rows(gi, gd, DT, radius=radius, top=topT, figures=fig)
            same_rows(radius_search(tree, Q, max_k, radius, T_dev), oi, od)  # a device-resident column-major pose
    assert empty > 0 and short > 0 and full > 0
    on = np.arange(0, 5000, 37)  # radius 0 at a target: the point itself and nothing else
    for max_k in (1, 10, 100):
        gi, gd = same_rows(radius_search(tree, dev(tgt[on]), max_k, 0.0), *orc.kdtree_radius(nodes, tgt[on], max_k, 0.0))
        assert np.array_equal(gi[:, 0], on) and (gd[:, 0] == 0).all() and (gi[:, 1:] == -1).all() and (gd[:, 1:] == FLT_MAX).all()
    print(f"device radius, leaf {leaf}: {fig}; rows empty / short / full = {empty} / {short} / {full}, ambiguous {ambiguous}")


@pytest.mark.parametrize("leaf", [16, 5])
def test_ties_at_long_lists_first_visited_wins(sp, orc, cloud, leaf):
    """Every point stored twice: each distance comes in a pair, and which of the two stands first is the traversal's doing
    (kdtree.hpp:119-137, strict '<'), not the index's — so this equals the oracle's tree and not a brute force's order."""
    tgt, qry, _, _ = cloud
    twice = np.concatenate([tgt[:2500], tgt[:2500]])
    tree = sp.KDTree.build(dev(twice), leaf)
    gi, gd = same_rows(tree.knn_search(dev(qry), 60), *orc.kdtree_knn(orc.kdtree_build(twice, leaf), qry, 60))
    Y.check_rows(gi, gd, Y.brute_d2(qry, twice))
    twin = np.sort(gi % 2500, axis=1)
    assert (gd[:, 0::2] == gd[:, 1::2]).all() and (twin[:, 0::2] == twin[:, 1::2]).all()
    assert (gi[:, 0::2] > gi[:, 1::2]).any()  # (the lowest index does not always come first)


@pytest.mark.parametrize("k", [10, 20])
def test_many_queries_take_the_unbatched_leaf_loop(sp, orc, cloud, k):
    """From 200 000 queries on, lists of 2..20 entries are searched by the BATCH_LEAF = false instantiation: 2048 distinct
    queries tiled to 200 704 must give the rows of the 2048-query launch (BATCH_LEAF = true) in every tile, and those the oracle's."""
    tgt, _, _, _ = cloud
    qry = orc.rng(8).uniform_points(2048, 5.5)
    tree = sp.KDTree.build(dev(tgt))
    nodes = orc.kdtree_build(tgt)
    Q = dev(qry)
    big = Q.repeat(98, 1)
    assert big.shape[0] == 200_704
    small = tree.knn_search(Q, k)
    same_rows(small, *orc.kdtree_knn(nodes, qry, k))
    r = tree.knn_search(big, k)
    assert (r.indices.view(98, 2048, k) == small.indices[None]).all() and (r.distances.view(98, 2048, k) == small.distances[None]).all()
    small = radius_search(tree, Q, k, 1.0)
    same_rows(small, *orc.kdtree_radius(nodes, qry, k, 1.0))
    r = radius_search(tree, big, k, 1.0)
    assert (r.indices.view(98, 2048, k) == small.indices[None]).all() and (r.distances.view(98, 2048, k) == small.distances[None]).all()


@pytest.fixture(scope="module")
def deep(orc):
    tgt, qry = Y.far_stack_cloud(orc)
    return tgt, qry, orc.knn_bruteforce(qry, tgt, 10)[0]


@pytest.mark.parametrize("leaf", [1, 2])
def test_far_stack_overflow_drops_what_the_reference_drops(sp, orc, deep, leaf):
    """300 000 points in leaves of one or two: deeper than the 16 far-stack entries. The reference drops pushes beyond them
    silently (kdtree.hpp:545-549) and so must the kernel, the same entries: bit for bit the oracle's rows, which are no longer
    the nearest neighbours (at least 5 % of the k = 10 rows differ from brute force; tests/test_oracle_kdtree_f64.py: 47-52 %)."""
    tgt, qry, bi = deep
    tree = sp.KDTree.build(dev(tgt), leaf)
    nodes = orc.kdtree_build(tgt, leaf)
    Q = dev(qry)
    for k in (1, 10, 60):
        gi, gd = same_rows(tree.knn_search(Q, k), *orc.kdtree_knn(nodes, qry, k))
        Y.check_rows(gi, gd, Y.gathered_d2(qry, tgt, gi), complete=False, n=len(tgt))
        if k == 10:
            differ = (gi != bi).any(1).mean()
            print(f"device far stack, leaf {leaf}: {100 * differ:.1f} % of k = 10 rows differ from brute force")
            assert differ >= 0.05
    gi, gd = same_rows(radius_search(tree, Q, 30, 0.6), *orc.kdtree_radius(nodes, qry, 30, 0.6))
    Y.check_rows(gi, gd, Y.gathered_d2(qry, tgt, gi), radius=0.6, complete=False, n=len(tgt))


def test_lazy_delete_at_long_lists(sp, orc, cloud):
    tgt, qry, _, _ = cloud
    fig = Y.Figures()
    tree = sp.KDTree.build(dev(tgt))
    nodes = orc.kdtree_build(tgt)
    Q = dev(qry)
    cur = tgt
    for flags in Y.removals(len(tgt)):
        new_idx = np.where(flags == 1, np.cumsum(flags) - 1, -1).astype(np.int32)
        tree.remove_nodes_by_flags(dev(flags), dev(new_idx))
        orc.kdtree_remove_by_flags(nodes, flags, new_idx)
        cur = cur[flags == 1]
        D = Y.brute_d2(qry, cur)  # the kept points under their new indices
        for k in (40, 100):
            gi, gd = same_rows(tree.knn_search(Q, k), *orc.kdtree_knn(nodes, qry, k))
            Y.check_rows(gi, gd, D, figures=fig)
        gi, gd = same_rows(radius_search(tree, Q, 100, 2.0), *orc.kdtree_radius(nodes, qry, 100, 2.0))
        Y.check_rows(gi, gd, D, radius=2.0, figures=fig)
    print(f"device after lazy deletes: {fig}")


def test_non_finite_queries_get_padding_rows(sp, orc, cloud):
    """A query with a NaN or inf coordinate, or one whose square overflows, has no neighbours: every entry (-1, FLT_MAX), as
    knn_search_bruteforce and every other structure give — whichever of them the seam picks for a call, the answer is the
    same. The reference's tree writes NaN distances for k > 1 here (tests/test_oracle_kdtree_f64.py)."""
    tgt, qry, _, _ = cloud
    q = np.concatenate([Y.non_finite_queries(), qry[:61]])
    P, Q = dev(tgt), dev(q)
    T = orc.se3_exp(TWIST)
    trees = [sp.KDTree.build(P), sp.KDTree.build(P, 5), sp.KDTree.build(P, accelerate=True)]
    for tree in trees:
        for k in (1, 5, 60):
            for transT in (None, T, pose_on_device(T)):
                gi, gd = host(tree.knn_search(Q, k, transT))
                assert (gi[:3] == -1).all() and (gd[:3] == FLT_MAX).all()
                assert (gi[3:] >= 0).all()  # (the finite queries in the same wave are searched as ever)
            if k <= 20:
                bi, bd = host(sp.knn_search_bruteforce(Q, P, k))
                gi, gd = host(tree.knn_search(Q, k))
                assert np.array_equal(gi[:3], bi[:3]) and np.array_equal(gd[:3], bd[:3]) and np.array_equal(gd, bd)
        for max_k in (1, 10, 60):
            gi, gd = host(radius_search(tree, Q, max_k, 2.0))
            assert (gi[:3] == -1).all() and (gd[:3] == FLT_MAX).all()


def test_argument_checks(sp, orc, cloud):
    tgt, qry, _, _ = cloud
    P, Q = dev(tgt), dev(qry)
    for leaf in (0, 4097):
        with pytest.raises(sp.SpError, match="leaf_threshold"):
            sp.KDTree.build(P, leaf)
        with pytest.raises(sp.SpError, match="leaf_threshold"):  # at build(), also where the reference's tree is built later
            sp.KDTree.build(P, leaf, accelerate=True)
        with pytest.raises(sp.SpError, match="leaf_threshold"):
            sp.KDTree.build(P[:500].contiguous(), leaf, accelerate=True)
    assert sp.KDTree.build(P, 4096).knn_search(Q, 2).indices.min() >= 0
    L = sp._lib.lib()
    idx = torch.full((len(qry), 101), -7, dtype=torch.int32, device="cuda")
    d2 = torch.zeros((len(qry), 101), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    plain, seam = sp.KDTree.build(P), sp.KDTree.build(P, accelerate=True)
    calls = (lambda: L.sp_kdtree_search(plain._h, ptr(Q), len(qry), 101, None, 0, ptr(idx), ptr(d2), st),
             lambda: L.sp_kdtree_radius_search(plain._h, ptr(Q), len(qry), 101, 1.0, None, 0, ptr(idx), ptr(d2), st),
             lambda: L.sp_knn_tree_search(seam._h, ptr(Q), len(qry), 101, None, 0, 0, ptr(idx), ptr(d2), st),
             lambda: L.sp_knn_tree_radius_search(seam._h, ptr(Q), len(qry), 101, 1.0, None, 0, ptr(idx), ptr(d2), st))
    for call in calls:  # the C entry points themselves (the Python class checks k before it calls them)
        with pytest.raises(sp.SpError, match="too large"):
            sp._lib.check(call())
    torch.cuda.synchronize()
    assert (idx == -7).all()  # nothing was launched
    for tree in (plain, seam):
        with pytest.raises(sp.SpError, match="too large"):
            tree.knn_search(Q, 101)
        with pytest.raises(sp.SpError, match="too large"):
            tree.radius_search_async(Q, 101, 1.0, sp.KNNResult())
        assert tree.knn_search(Q, 100).indices.min() >= 0


# ------------------------------------------------------------------------------------------ the sp_knn_tree seam
SEAM_KS = (7, 8, 20, 21, 32, 33, 100)


def expected_backend(n, nq, k, transform, own, grid_fits):
    """The rule at the top of csrc/knn_tree.hip, restated."""
    if n < 1024 or k > 32:
        return "kdtree"
    if own and 8 <= k <= 20 and n >= 32768 and grid_fits:
        return "grid"
    one_launch = 256 <= n <= 12032 and nq * n <= 80_000_000  # (sp_knn_bruteforce keeps the cloud in LDS)
    if k <= 20 and not transform and nq <= 65536 and (one_launch or (2048 <= n <= 16384 and n >= 256 * k)):
        return "bruteforce"
    return "bvh"


def seam_cloud(orc, name):
    if name == "clustered":
        return nonuniform_cloud(40_000, seed=5), False
    return orc.rng(int(name)).uniform_points(int(name), 5.0), True


@pytest.mark.parametrize("name", ["1023", "1024", "6000", "40000", "clustered"])
def test_seam_every_backend_answers_with_the_same_lists(sp, orc, name):
    pts, grid_fits = seam_cloud(orc, name)
    n = len(pts)
    rs = np.random.RandomState(2)
    ext = pts[rs.choice(n, 300, replace=False)].copy()
    ext[:, :3] += rs.normal(0, 0.05, (300, 3)).astype(np.float32)
    T = orc.se3_exp(np.float32([0.02, -0.03, 0.01, 0.1, -0.05, 0.08]))
    extT = Y.transformed_f64_checked(ext, T, orc.transform_points(ext, T))
    rows = np.sort(rs.choice(n, 300, replace=False))  # the own cloud's rows that are held to the yardstick
    P, E = dev(pts), dev(ext)
    tree = sp.KDTree.build(P, accelerate=True)
    nodes = orc.kdtree_build(pts)
    fig = Y.Figures()
    modes = (("own", P, None, Y.brute_d2(pts[rows], pts), rows, pts[rows]), ("external", E, None, Y.brute_d2(ext, pts), slice(None), ext),
             ("transform", E, T, Y.brute_d2(extT, pts), slice(None), ext))
    seen = set()
    for label, Qd, transT, D, sel, q_host in modes:
        top = Y.top_sorted(D, 100)
        got = {}
        for k in SEAM_KS:
            want = expected_backend(n, Qd.shape[0], k, transT is not None, label == "own", grid_fits)
            assert tree.backend_for(Qd, k, transT) == want, (label, k)
            seen.add(want)
            gi, gd = host(tree.knn_search(Qd, k, transT))
            Y.check_rows(gi[sel], gd[sel], D, top=top, figures=fig)
            if want == "kdtree":
                oi, od = orc.kdtree_knn(nodes, q_host, k, transT)
                assert np.array_equal(gd[sel], od) and np.array_equal(gi[sel], oi)
            got[k] = (gi[sel], gd[sel])
        # across the switch from the hierarchy (k = 32) to the reference's tree (k = 33): the same 32 nearest
        (i32, d32), (i33, d33) = got[32], got[33]
        assert np.array_equal(d33[:, :32], d32)
        distinct = (np.diff(d33, axis=1) > 0).all(1)  # (tie-free rows: the indices too)
        assert distinct.mean() > 0.9 and np.array_equal(i33[distinct, :32], i32[distinct])
        if label != "own":
            # (uniform clouds: about 36 points in the ball, so that lists of 40 come out full, cut short and below 32)
            radius = 0.4 if name == "clustered" else (36 / (n / 1000 * 4.18879)) ** (1 / 3)
            (i32, d32), (i40, d40) = host(radius_search(tree, Qd, 32, radius, transT)), host(radius_search(tree, Qd, 40, radius, transT))
            Y.check_rows(i32, d32, D, radius=radius, top=top, figures=fig)
            Y.check_rows(i40, d40, D, radius=radius, top=top, figures=fig)
            assert np.array_equal(d40[:, :32], d32)
            oi, od = orc.kdtree_radius(nodes, q_host, 40, radius, transT)
            assert np.array_equal(d40, od) and np.array_equal(i40, oi)
            n40 = (i40 >= 0).sum(1)
            assert (n40 == 40).any() and (n40 < 32).any()
    assert seen == {"1023": {"kdtree"}, "1024": {"kdtree", "bruteforce", "bvh"}, "6000": {"kdtree", "bruteforce", "bvh"},
                    "40000": {"kdtree", "grid", "bvh"}, "clustered": {"kdtree", "bvh"}}[name]
    print(f"seam, {name} points: {fig}")


def test_seam_long_radius_lists_replay_lazy_deletes(sp, orc):
    """radius_search with max_k > 32 goes to the reference's tree. On a tree whose nodes were removed twice while only the
    hierarchy existed, that tree is built from the original points at this call and replays both removals first: the rows are
    the oracle's tree's after the same removals, and pass the yardstick over the kept points under their new indices."""
    pts = orc.rng(99).uniform_points(6000, 5.0)
    qry = orc.rng(7).uniform_points(300, 5.0)
    Q = dev(qry)
    fig = Y.Figures()
    tree = sp.KDTree.build(dev(pts), accelerate=True)
    nodes = orc.kdtree_build(pts)
    cur = pts
    for flags in Y.removals(len(pts)):
        new_idx = np.where(flags == 1, np.cumsum(flags) - 1, -1).astype(np.int32)
        tree.remove_nodes_by_flags(dev(flags), dev(new_idx))
        orc.kdtree_remove_by_flags(nodes, flags, new_idx)
        cur = cur[flags == 1]
    D = Y.brute_d2(qry, cur)
    # (this call builds the reference's tree)
    gi, gd = same_rows(radius_search(tree, Q, 40, 1.5), *orc.kdtree_radius(nodes, qry, 40, 1.5))
    Y.check_rows(gi, gd, D, radius=1.5, figures=fig)
    n40 = (gi >= 0).sum(1)
    assert (n40 == 40).any() and (n40 < 40).any()
    hi, hd = host(radius_search(tree, Q, 32, 1.5))  # the hierarchy, after the same removals
    Y.check_rows(hi, hd, D, radius=1.5, figures=fig)
    assert np.array_equal(gd[:, :32], hd)
    gi, gd = same_rows(tree.knn_search(Q, 100), *orc.kdtree_knn(nodes, qry, 100))
    Y.check_rows(gi, gd, D, figures=fig)
    print(f"seam after lazy deletes: {fig}")


def test_seam_keeps_the_leaf_threshold_for_the_reference_tree(sp, orc):
    pts = orc.rng(99).uniform_points(6000, 5.0)
    qry = orc.rng(7).uniform_points(300, 5.0)
    tree = sp.KDTree.build(dev(pts), 5, accelerate=True)
    nodes5 = orc.kdtree_build(pts, 5)
    gi, gd = same_rows(tree.knn_search(dev(qry), 40), *orc.kdtree_knn(nodes5, qry, 40))
    Y.check_rows(gi, gd, Y.brute_d2(qry, pts))
    # leaf 5 and leaf 16 visit in different orders: with every point stored twice the tie order tells them apart
    twice = np.concatenate([pts[:3000], pts[:3000]])
    tree = sp.KDTree.build(dev(twice), 5, accelerate=True)
    i5, d5 = orc.kdtree_knn(orc.kdtree_build(twice, 5), qry, 40)
    i16, _ = orc.kdtree_knn(orc.kdtree_build(twice, 16), qry, 40)
    assert not np.array_equal(i5, i16)
    same_rows(tree.knn_search(dev(qry), 40), i5, d5)
