"""The engineered cascades of tests/bvh_walks.py on the host mirror alone: the clouds produce the stack depths the GPU tests
(tests/test_gpu_bvh_walks.py) state, and every rare branch of csrc/bvh.hip's walks — LDS stack only, arena slot in use, both
stacks exactly full, handed on, rescanned — is reached by at least one query of the sets those tests send. Inputs that reach no
rare branch fail here instead of passing silently on the device."""
import numpy as np
import pytest

import bvh_walks as W

PUSHES = (20, 21, 46, 48, 50)


@pytest.fixture(scope="module")
def trees():
    return {p: W.Tree(W.cascade_by_pushes(p)) for p in PUSHES}


def test_fma32_is_the_fused_operation():
    # products and sums that a float64 detour rounds twice: 1 + 2^-24 + 2^-60 must round up, the float64 sum alone loses the tail
    a, b = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)  # a * b = 1 + 2^-11 + 2^-24
    assert W.fma32(a, b, np.float32(2.0 ** -60))[0] == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert W.fma32(a, b, np.float32(-2.0 ** -60))[0] == np.float32(1 + 2.0 ** -11)
    assert W.fma32(a, b, np.float32(0))[0] == np.float32(1 + 2.0 ** -11)  # the tie goes to even
    rs = np.random.RandomState(0)
    x, y, z = (rs.standard_normal(1000).astype(np.float32) for _ in range(3))
    exact = x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)  # within half an ulp of float64 of the truth
    assert (np.abs(W.fma32(x, y, z).astype(np.float64) - exact) <= np.abs(exact) * 2.0 ** -24 * (1 + 1e-6)).all()


def test_dist2_restatement_equals_the_oracle(orc, trees):
    """The float32 distances the expected lists above k = 20 are made of, against knn_search_bruteforce's at k = 20: on a
    cascade with the external query set and on a random cloud (rounded squares and sums)."""
    g = orc.rng(4321)
    for tgt, qry in ((W.cascade_by_pushes(46), W.external_queries()), (g.uniform_points(700, 10.0), g.uniform_points(40, 10.0))):
        oi, od = orc.knn_bruteforce(qry, tgt, 20)
        bi, bd = W.brute_force(qry, tgt, 20)
        assert np.array_equal(oi, bi) and np.array_equal(od, bd)


def test_first_forty_morton_positions_are_origin_copies(trees):
    for p, t in trees.items():
        assert (t.pts[:40] == 0).all() and t.keys[:40] == [0] * 40
        assert t.idx[:40] == sorted(t.idx[:40])  # equal keys: by original index, so the 40 lowest indices come first
        flags, _ = W.lazy_delete_flags(W.cascade_by_pushes(p))
        assert sorted(np.flatnonzero(flags == 0).tolist()) == t.idx[:40]


def test_hierarchy_ranges_partition_the_points(trees):
    for t in trees.values():
        assert (t.first[0], t.last[0]) == (0, t.n - 1)
        for i in range(t.n - 1):
            f, s, l = t.first[i], t.split[i], t.last[i]
            assert f <= s < l and i in (f, l)
            for c, (cf, cl) in ((s, (f, s)), (s + 1, (s + 1, l))):
                if cl > cf:
                    assert (t.first[c], t.last[c]) == (cf, cl)


@pytest.mark.parametrize("k", [25, 32])
def test_pushes_of_the_origin_query(trees, k):
    origin = W.external_queries()[:1]
    for p, t in trees.items():
        (rec,), (handed, claims) = W.predict(t, origin, k)
        print(f"cascade{W.CASCADES[p]}: {t.n} points, k = {k}: {rec['pushes']} pushes, window positions valid {rec['valid']}, "
              f"claimed {rec['claimed']}, handed on {rec['handed_on']}, rescan {rec['rescan']}")
        assert rec["valid"] == 24 and rec["pushes"] == p
        assert rec["claimed"] == (p > W.LDS_STACK) and claims == int(p > W.LDS_STACK)
        assert rec["handed_on"] == (p > W.LDS_STACK + W.DEEP_STACK) == rec["rescan"] and handed == int(p > 48)
    assert [trees[p].n for p in (46, 48, 50)] == [964, 1156, 1924]


def test_the_sorted_insertion_kernel_alone_on_the_origin_query(trees):
    """With the heap kernel switched off the same descent runs on the 48-entry stack of bvh_search_kernel: full at 48, over at 50."""
    for p, t in trees.items():
        w = t.sorted_walk(t.geometry([0, 0, 0]), 25, W.sorted_kcap(25))
        assert w["max_stack"] == min(p, W.SEARCH_STACK) and w["overflow"] == (p > W.SEARCH_STACK)


def test_every_class_is_populated_by_the_gpu_tests_queries(trees):
    Q = W.external_queries()
    seen = {}
    for p, t in trees.items():
        for name, (q, k, radius) in {"knn25": (Q, 25, None), "knn32": (Q, 32, None), "radius32": (Q, 32, 1.0e5),
                                     "self32": (None, 32, None)}.items():
            recs, counts = W.predict(t, q, k, radius)
            seen[p, name] = W.classes(recs)
            print(f"{p} pushes, {name}: {sorted(seen[p, name])}, handed on {counts[0]}, arena claims {counts[1]}")
    for name in ("knn25", "knn32", "radius32", "self32"):
        assert seen[20, name] == {"lds"}
        assert seen[21, name] == {"lds", "arena"}
        assert seen[46, name] == {"lds", "arena"}
        assert seen[48, name] == {"lds", "arena", "full"}
        assert seen[50, name] == {"lds", "handed_on", "rescan"}


def test_every_heap_shape_goes_deep_after_the_lazy_delete():
    Q = W.external_queries()
    for p in (46, 50):
        cloud = W.cascade_by_pushes(p)
        t = W.Tree(cloud)
        t.remove_by_flags(*W.lazy_delete_flags(cloud))
        for k in (1, 5, 10, 21):
            recs, counts = W.predict(t, Q, k)
            print(f"{p} pushes after the delete, external k = {k}: pushes {[r['pushes'] for r in recs]}, counters {counts}")
            assert recs[0]["valid"] == 0 and recs[0]["pushes"] == p  # the origin: no valid window position, the whole chain
            assert ("arena" if p == 46 else "rescan") in W.classes(recs)
        for k in (5, 10, 21):
            recs, counts = W.predict(t, None, k)
            print(f"{p} pushes after the delete, self k = {k}: {sorted(W.classes(recs))}, counters {counts}")
            assert len(recs) == t.n - 40
        assert ("arena" if p == 46 else "rescan") in W.classes(recs)  # k = 21: the first kept origin copies see < 21 valid


def test_arena_exhaustion_prediction(trees):
    recs, counts = W.predict(trees[46], W.external_queries()[:1], 32, repeat=W.ARENA_MAX + 512)
    assert counts == (512, W.ARENA_MAX + 512)
