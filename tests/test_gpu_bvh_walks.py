"""csrc/bvh.hip's walks on the engineered deep trees of tests/bvh_walks.py: every stack boundary of bvh_walk (the last LDS entry
at 20 pushes, the first arena entry at 21, the arena in use at 46, both 48-entry stacks exactly full at 48, the hand-over and the
sorted-insertion kernel's rescan of all points at 50), every heap shape at depth after a lazy delete, an exhausted arena, and
degenerate extents and tiny trees. Every list is compared bit for bit — indices and distances — with a (distance,
index)-lexicographic brute force (the oracle's knn_search_bruteforce up to k = 20, the helper's float32 restatement above, held
to the oracle at k = 20 by tests/test_bvh_walks_cpu.py), with the heap kernel on and off, and the device's two walk counters
(queries handed on, arena slots asked for) with what the host mirror predicts for that very call.
tests/test_bvh_walks_cpu.py proves on the mirror alone that these inputs reach the branches named here."""
import functools

import numpy as np
import pytest

import bvh_walks as W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(r, rows=None):
    return r.indices[:rows].cpu().numpy(), r.distances[:rows].cpu().numpy()


@functools.lru_cache(maxsize=None)
def cascade(pushes):
    return W.cascade_by_pushes(pushes)  # (shared between the tests: nobody writes to it)


def expected(orc, qry, tgt, k, radius=None):
    if k <= 20 and radius is None:
        return orc.knn_bruteforce(qry, tgt, k)
    return W.brute_force(qry, tgt, k, radius)


def both(b, fn, want, counts=None, rows=None):
    """fn() with the sorted-insertion kernel alone and with the heap kernel: the same rows, equal to `want`; with the heap kernel
    the walk counters equal `counts` (the mirror's prediction), without it they are zero."""
    b._set_option("bvh_walk_counts", 1)
    b._set_option("bvh_self_heap", 0)
    ai, ad = host(fn(), rows)
    assert b._walk_counts() == (0, 0)
    b._set_option("bvh_self_heap", 1)
    ci, cd = host(fn(), rows)
    got = b._walk_counts()
    b._set_option("bvh_walk_counts", 0)
    assert np.array_equal(ai, want[0]) and np.array_equal(ad, want[1]), "sorted-insertion kernel differs from brute force"
    assert np.array_equal(ci, want[0]) and np.array_equal(cd, want[1]), "heap kernel differs from brute force"
    if counts is not None:
        print(f"    (handed on, arena claims): device {got}, mirror {counts}")
        assert got == counts, f"walk counters (handed on, arena claims): device {got}, mirror {counts}"


@pytest.mark.parametrize("pushes", [20, 21, 46, 48, 50])
def test_every_stack_boundary(sp, orc, pushes):
    cloud, qry = cascade(pushes), W.external_queries()
    tree = W.Tree(cloud)
    b = sp.BVH.build(dev(cloud))
    Q = dev(qry)
    seen = set()
    for k in (25, 32):
        recs, counts = W.predict(tree, qry, k)
        seen |= W.classes(recs)
        assert recs[0]["pushes"] == pushes
        both(b, lambda: b.knn_search(Q, k), expected(orc, qry, cloud, k), counts)
    recs, counts = W.predict(tree, qry, 32, radius=1.0e5)
    seen |= W.classes(recs)
    both(b, lambda: b.radius_search(Q, 32, 1.0e5), expected(orc, qry, cloud, 32, 1.0e5), counts)
    recs, counts = W.predict(tree, None, 32)
    seen |= W.classes(recs)
    both(b, lambda: b.self_knn(32), expected(orc, cloud, cloud, 32), counts)
    assert seen == {20: {"lds"}, 21: {"lds", "arena"}, 46: {"lds", "arena"}, 48: {"lds", "arena", "full"},
                    50: {"lds", "handed_on", "rescan"}}[pushes]


@pytest.mark.parametrize("pushes", [46, 50])
def test_every_heap_shape_at_depth_after_a_lazy_delete(sp, orc, pushes):
    cloud, qry = cascade(pushes), W.external_queries()
    flags, new_idx = W.lazy_delete_flags(cloud)
    tree = W.Tree(cloud)
    tree.remove_by_flags(flags, new_idx)
    b = sp.BVH.build(dev(cloud))
    b.remove_nodes_by_flags(dev(flags), dev(new_idx))
    kept = cloud[flags == 1]
    Q = dev(qry)
    for k in (1, 5, 10, 21):
        recs, counts = W.predict(tree, qry, k)
        assert recs[0]["pushes"] == pushes and recs[0]["valid"] == 0
        both(b, lambda: b.knn_search(Q, k), expected(orc, qry, kept, k), counts)
    for k in (5, 10, 21):
        recs, counts = W.predict(tree, None, k)
        both(b, lambda: b.self_knn(k), expected(orc, kept, kept, k), counts, rows=len(kept))  # (rows behind the kept: not written)


def test_arena_exhaustion(sp, orc):
    cloud = cascade(46)
    nq = W.ARENA_MAX + 512
    one = W.external_queries()[:1]
    tree = W.Tree(cloud)
    b = sp.BVH.build(dev(cloud))
    want = expected(orc, one, cloud, 32)
    both(b, lambda: b.knn_search(dev(one), 32), want, W.predict(tree, one, 32)[1])
    Q = dev(np.repeat(one, nq, axis=0))
    counts = W.predict(tree, one, 32, repeat=nq)[1]
    assert counts == (512, nq)
    wi, wd = dev(want[0]), dev(want[1])
    for sort_queries in (0, 1):  # (below the 400 k of the sort: nothing may differ)
        b._set_option("bvh_sort_queries", sort_queries)
        for heap in (0, 1):
            b._set_option("bvh_self_heap", heap)
            b._set_option("bvh_walk_counts", 1)
            r = b.knn_search(Q, 32)
            got = b._walk_counts()
            b._set_option("bvh_walk_counts", 0)
            assert bool((r.indices == wi).all()) and bool((r.distances == wd).all()), (sort_queries, heap)
            assert got == (counts if heap else (0, 0)), (sort_queries, heap, got)
    b._set_option("bvh_sort_queries", 1)


def search_all(sp, orc, tgt, qry, ks):
    """Own points and external queries, heap kernel on and off, against brute force."""
    b = sp.BVH.build(dev(tgt))
    Q = dev(qry)
    for k in ks:
        both(b, lambda: b.knn_search(Q, k), expected(orc, qry, tgt, k))
        both(b, lambda: b.self_knn(k), expected(orc, tgt, tgt, k))


def test_one_point_five_thousand_times(sp, orc):
    """No extent on any axis: every key is 0, the hierarchy splits by sorted position alone, every box is the point. The 20
    lowest indices, from every copy and from outside."""
    p = np.float32([1.5, -2.25, 3.0, 1.0])
    tgt = np.repeat(p[None], 5000, axis=0)
    qry = np.stack([p, p + np.float32([1, 0, 0, 0]), p - np.float32([0, 7, 0.5, 0]), np.float32([np.nan, 0, 0, 1])])
    b = sp.BVH.build(dev(tgt))
    for heap in (0, 1):
        b._set_option("bvh_self_heap", heap)
        s = b.self_knn(20)
        assert bool((s.indices == dev(np.arange(20, dtype=np.int32))).all()) and bool((s.distances == 0).all())
        r = host(b.knn_search(dev(qry), 20))
        want = orc.knn_bruteforce(qry, tgt, 20)
        assert np.array_equal(r[0], want[0]) and np.array_equal(r[1], want[1])
        assert (r[0][:3] == np.arange(20)).all()
    search_all(sp, orc, tgt[:700], qry, (2, 32))


def test_planar_collinear_and_corner_clouds(sp, orc):
    rs = np.random.RandomState(5)
    base = np.ones((600, 4), np.float32)
    base[:, :3] = rs.uniform(-3, 3, (600, 3))
    qry = np.ones((64, 4), np.float32)
    qry[:, :3] = rs.uniform(-4, 4, (64, 3))
    qry[:8] = base[:8]
    planar = base.copy()
    planar[:, 2] = 0.75  # one axis without extent
    line = base.copy()
    line[:, 1:3] = [0.75, -1.5]  # two
    line[100:140] = line[100]  # ... and ties along it
    corner = base.copy()  # points exactly on the box's upper faces, edges and corner: cell 65535 clamped to 65534
    hi = corner[:, :3].max(0)
    for i, axes in enumerate(((0,), (1,), (2,), (0, 1), (1, 2), (0, 2), (0, 1, 2), (0, 1, 2))):
        corner[40 * i:40 * i + 25, axes] = hi[list(axes)]
    for tgt in (planar, line, corner):
        search_all(sp, orc, tgt, np.concatenate([qry, tgt[-4:]]), (1, 6, 20, 27))


@pytest.mark.parametrize("n", [16, 17, 18, 33])
def test_tiny_trees_around_the_leaf_size(sp, orc, n):
    g = orc.rng(100 + n)
    tgt, qry = g.uniform_points(n, 2.0), g.uniform_points(40, 2.5)
    qry[:4] = tgt[:4]
    qry[5, 1] = np.nan
    search_all(sp, orc, tgt, qry, (1, 2, 5, 16, 20, 21, 32))


@pytest.mark.parametrize("n", [4, 17, 40])
def test_extent_that_overflows_float32(sp, orc, n):
    """Two finite points 6e38 apart (the box's extent and their squared distance overflow float32) next to NaN points. A
    neighbour at an infinite float32 distance is none: knn/bruteforce.hpp:46-92 starts every slot at max() and takes a candidate
    only when its distance is below the slot's, so +inf never enters — rows end in (-1, FLT_MAX)."""
    tgt = np.full((n, 4), np.nan, np.float32)
    tgt[:, 3] = 1.0
    tgt[1, :3] = [3.0e38, 0, 0]
    tgt[n - 2, :3] = [-3.0e38, 1.0, 0]
    qry = np.float32([[3.0e38, 0, 0, 1], [0, 0, 0, 1], [-1.0e38, 0, 0, 1], [-3.0e38, 1.0, 0, 1], [np.inf, 0, 0, 1]])
    want = orc.knn_bruteforce(qry, tgt, 2)
    assert want[0].tolist() == [[1, -1], [-1, -1], [-1, -1], [n - 2, -1], [-1, -1]]
    assert np.array_equal(W.brute_force(qry, tgt, 2)[0], want[0])
    search_all(sp, orc, tgt, qry, (1, 2, 3, 32))
