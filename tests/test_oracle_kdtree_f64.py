"""The oracle's KD-tree (oracle/oracle_knn.hpp: the reference's build, traversal, radius search and lazy delete restated on the
CPU) against the float64 yardstick of f64_knn.py, in the regions tests/test_gpu_kdtree_seam.py leans on it: every list class
of the reference's dispatch and its edges (k = 1, 2, 10 | 11, 20 | 21, 50 | 51, 100), leaf sizes 1, 5, 16, 33 and 4096 (the
root itself a leaf), radius searches with up to 100 entries, lazy deletes, the 16-entry far stack when it overflows, and the
reference's answer to a non-finite query. The device tests compare with this oracle bit for bit; this file is what says the
oracle's lists are right (or, for the far stack and the NaN rows, exactly how they are wrong)."""
import numpy as np
import pytest

import f64_knn as Y

FLT_MAX = Y.FLT_MAX
KS = (1, 2, 10, 11, 20, 21, 50, 51, 100)
RADII = (0.3, 1.0, 2.0, 4.0)  # at 5 points per unit volume: about 0.6, 21, 170 and 1300 points in the ball


@pytest.fixture(scope="module")
def cloud(orc):
    tgt, qry = Y.matrix_cloud(orc)
    D = Y.brute_d2(qry, tgt)
    return tgt, qry, D, Y.top_sorted(D, 100)


@pytest.mark.parametrize("leaf", [1, 5, 16, 33, 4096])
def test_oracle_kdtree_knn_every_list_class_and_leaf_size(orc, cloud, leaf):
    tgt, qry, D, top = cloud
    fig = Y.Figures()
    nodes = orc.kdtree_build(tgt, leaf)
    for k in KS:
        idx, d = orc.kdtree_knn(nodes, qry, k)
        Y.check_rows(idx, d, D, top=top, figures=fig)
    small = tgt[:150]  # one leaf block under the root
    nodes = orc.kdtree_build(small, 4096)
    assert len(nodes) // 32 == 151
    Ds = D[:, :150]
    for k in KS:
        idx, d = orc.kdtree_knn(nodes, qry, k)
        Y.check_rows(idx, d, Ds, figures=fig)
    n = Y.full_leaves_size(leaf)  # every leaf block full to its last slot
    nodes = orc.kdtree_build(tgt[:n], leaf)
    topn = Y.top_sorted(D[:, :n], 100)
    for k in KS:
        idx, d = orc.kdtree_knn(nodes, qry, k)
        Y.check_rows(idx, d, D[:, :n], top=topn, figures=fig)
    for max_k in (1, 10, 100):
        idx, d = orc.kdtree_radius(nodes, qry, max_k, 1.5)
        Y.check_rows(idx, d, D[:, :n], radius=1.5, top=topn, figures=fig)
    idx, d = orc.kdtree_knn(orc.kdtree_build(tgt[:17], leaf), qry, 100)  # fewer points than k: padded rows
    Y.check_rows(idx, d, D[:, :17], figures=fig)
    assert ((idx >= 0).sum(1) == 17).all()
    print(f"oracle kNN, leaf {leaf}: {fig}")


@pytest.mark.parametrize("leaf", [5, 16])
def test_oracle_kdtree_radius_up_to_100_entries(orc, cloud, leaf):
    tgt, qry, D, top = cloud
    fig = Y.Figures()
    nodes = orc.kdtree_build(tgt, leaf)
    T = orc.se3_exp(np.float32([0.05, -0.1, 0.02, 0.2, -0.1, 0.1]))
    qT = Y.transformed_f64_checked(qry, T, orc.transform_points(qry, T))
    DT = Y.brute_d2(qT, tgt)
    empty = short = full = ambiguous = 0
    for max_k in (1, 10, 20, 50, 100):
        for radius in RADII:
            idx, d = orc.kdtree_radius(nodes, qry, max_k, radius)
            ambiguous += Y.check_rows(idx, d, D, radius=radius, top=top, figures=fig)
            n = (idx >= 0).sum(1)
            empty, short, full = empty + (n == 0).sum(), short + ((n > 0) & (n < max_k)).sum(), full + (n == max_k).sum()
            idx, d = orc.kdtree_radius(nodes, qry, max_k, radius, T)
            ambiguous += Y.check_rows(idx, d, DT, radius=radius, figures=fig)
    assert empty > 0 and short > 0 and full > 0
    on = np.arange(0, 5000, 37)  # radius 0 at a target: the point itself
    idx, d = orc.kdtree_radius(nodes, tgt[on], 10, 0.0)
    assert np.array_equal(idx[:, 0], on) and (d[:, 0] == 0).all() and (idx[:, 1:] == -1).all() and (d[:, 1:] == FLT_MAX).all()
    print(f"oracle radius, leaf {leaf}: {fig}; rows empty / short / full = {empty} / {short} / {full}, ambiguous {ambiguous}")


def test_oracle_kdtree_lazy_delete_at_long_lists(orc, cloud):
    tgt, qry, _, _ = cloud
    fig = Y.Figures()
    nodes = orc.kdtree_build(tgt, 16)
    cur = tgt
    for flags in Y.removals(len(tgt)):
        new_idx = np.where(flags == 1, np.cumsum(flags) - 1, -1).astype(np.int32)
        orc.kdtree_remove_by_flags(nodes, flags, new_idx)
        cur = cur[flags == 1]
        D = Y.brute_d2(qry, cur)
        for k in (40, 100):
            idx, d = orc.kdtree_knn(nodes, qry, k)
            Y.check_rows(idx, d, D, figures=fig)
        idx, d = orc.kdtree_radius(nodes, qry, 100, 2.0)
        Y.check_rows(idx, d, D, radius=2.0, figures=fig)
    print(f"oracle after lazy deletes: {fig}")


@pytest.mark.parametrize("leaf", [1, 2])
def test_oracle_far_stack_overflows_and_drops_subtrees(orc, leaf):
    """300 000 points in leaves of one or two: the tree is deeper than the 16 far-stack entries, pushes beyond them are dropped
    (kdtree.hpp:206, 437, 545-549) and the lists are no longer the nearest neighbours. What is listed is still a valid list;
    at least 5 % of the k = 10 rows must differ from brute force (52 % and 47 % on this cloud), so the case cannot quietly
    stop overflowing."""
    tgt, qry = Y.far_stack_cloud(orc)
    nodes = orc.kdtree_build(tgt, leaf)
    idx, d = orc.kdtree_knn(nodes, qry, 10)
    Y.check_rows(idx, d, Y.gathered_d2(qry, tgt, idx), complete=False, n=len(tgt))
    bi, bd = orc.knn_bruteforce(qry, tgt, 10)
    differ = (idx != bi).any(1).mean()
    i1, _ = orc.kdtree_knn(nodes, qry, 1)
    print(f"far stack, leaf {leaf}: {100 * differ:.1f} % of k = 10 rows differ from brute force, "
          f"{(i1[:, 0] != bi[:, 0]).sum()} of {len(qry)} at k = 1")
    assert differ >= 0.05
    assert (d >= bd).all()  # a dropped subtree can only lose nearer points
    shallow = tgt[:70_000]  # depth 17 with one-point leaves, and nothing is dropped yet
    idx, d = orc.kdtree_knn(orc.kdtree_build(shallow, leaf), qry, 10)
    bi, bd = orc.knn_bruteforce(qry, shallow, 10)
    assert np.array_equal(d, bd)


def test_oracle_kdtree_non_finite_queries_follow_the_reference(orc, cloud):
    """The reference's insert_to_bestK (kdtree.hpp:119-137) leaves with `dist_sq >= bestK[k-1]`, which a NaN never satisfies:
    for k > 1 a query with a NaN coordinate, or an inf one (0 * inf in the query transform), gets real indices with NaN
    distances. For k = 1 the comparison is `dist_sq < best`, and the row stays (-1, FLT_MAX); so does every row of a query
    whose squared coordinate overflows (the distance is +inf, never below FLT_MAX). The device kernels write (-1, FLT_MAX)
    in all of these cases (tests/test_gpu_kdtree_seam.py): this test records the reference's side of that."""
    tgt, _, _, _ = cloud
    nodes = orc.kdtree_build(tgt, 16)
    q = Y.non_finite_queries()
    for k in (5, 60):
        idx, d = orc.kdtree_knn(nodes, q, k)
        # every point the walk meets is inserted (no far child is pushed: `split < NaN` is false, so that is one path from
        # the root to a leaf): NaN distances with real indices, k = 5 full, k = 60 with the slots that were never reached behind
        nan = np.isnan(d[:2])
        assert nan[:, :5].all() and (nan[:, 1:] <= nan[:, :-1]).all()
        assert ((idx[:2] >= 0) & (idx[:2] < len(tgt)))[nan].all()
        assert (idx[:2][~nan] == -1).all() and (d[:2][~nan] == FLT_MAX).all()
        assert (idx[2] == -1).all() and (d[2] == FLT_MAX).all()
    idx, d = orc.kdtree_knn(nodes, q, 1)
    assert (idx == -1).all() and (d == FLT_MAX).all()
    idx, d = orc.kdtree_radius(nodes, q, 10, 2.0)  # `d <= radius_sq` is false for a NaN: nothing is counted
    assert (idx == -1).all() and (d == FLT_MAX).all()
