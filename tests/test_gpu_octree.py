"""Device-built octree (csrc/octree.hip, sp_octree_*, api.Octree, knn::Octree): exact kNN for k <= 100 against the CPU oracle —
orc.knn_bruteforce up to k = 20 (the same tie rule: indices and distances bit for bit), the oracle's KD-tree above (distances
bit for bit, indices equal on clouds the test first shows to be free of ties) — on the reference's test cloud
(cpp/tests/test_kdtree.cpp:21-25), across structure parameters, on a cloud whose density varies by four orders of magnitude, at
the edges, after lazy removal; the exported structure itself; the compiler's resource report; the C++ facade."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nonuniform_cloud(n, seed=7):
    """tests/test_gpu_bvh.py's cloud: points on three planes (a floor and two walls, noisy), plus a dense cluster holding a fifth
    of the points in a 20 cm ball: density varies by more than four orders of magnitude."""
    rs = np.random.RandomState(seed)
    m = n // 5
    parts = []
    for axis in range(3):
        p = rs.uniform(-40, 40, (m, 3))
        p[:, axis] = rs.normal(0.0, 0.01, m)
        parts.append(p)
    parts.append(rs.uniform(-40, 40, (n - 4 * m, 3)) * np.array([1.0, 1.0, 0.1]))
    c = rs.normal(0.0, 1.0, (m, 3))
    parts.append(np.array([3.0, -2.0, 1.0]) + 0.2 * c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-9) * rs.uniform(0, 1, (m, 1)) ** (1 / 3))
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = np.concatenate(parts)[:n].astype(np.float32)
    return pts


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def reference_cloud(orc):
    """orc.rng(1234): 1000 targets, then 100 queries, range 10."""
    def make():
        g = orc.rng(1234)
        return g.uniform_points(1000, 10.0), g.uniform_points(100, 10.0)
    return cached("reference", make)


def dense_cloud():
    def make():
        pts = nonuniform_cloud(20000)
        return pts, np.ascontiguousarray(pts[::10])
    return cached("nonuniform", make)


def oracle_rows(orc, name, tgt, qry, k):
    """The expected rows and, per row, whether the LAST index is compared (False only at k = 100 where the 101st neighbour is
    too close to tell). k <= 20: brute force, the same tie rule. Above: the oracle's KD-tree, whose tie order is first-visited —
    so the cloud is first shown to be free of ties, with the (k + 1)-th neighbour included (k = 100: the oracle refuses 101, so
    inner ties only, and the float64 gap between the 100th and the 101st distance decides about the last index)."""
    def make():
        every = np.ones(len(qry), bool)
        if k <= 20:
            return orc.knn_bruteforce(qry, tgt, k) + (every,)
        nodes = cached(("kdtree", name), lambda: orc.kdtree_build(tgt))
        if k < 100:
            i1, d1 = orc.kdtree_knn(nodes, qry, k + 1)
            assert (np.diff(d1, axis=1) > 0).all(), "the cloud has a tie: choose another"
            return np.ascontiguousarray(i1[:, :k]), np.ascontiguousarray(d1[:, :k]), every
        oi, od = orc.kdtree_knn(nodes, qry, k)
        assert (np.diff(od, axis=1) > 0).all(), "the cloud has a tie: choose another"
        sure = np.empty(len(qry), bool)
        t64 = tgt[:, :3].astype(np.float64)
        for a in range(0, len(qry), 250):
            d = ((qry[a:a + 250, None, :3].astype(np.float64) - t64[None]) ** 2).sum(-1)
            near = np.partition(d, (k - 1, k), axis=1)
            sure[a:a + 250] = (near[:, k] - near[:, k - 1]) > 1e-5 * near[:, k]
        assert (~sure).mean() <= 0.01
        return oi, od, sure
    return cached(("rows", name, k), make)


def assert_rows(res, expected):
    oi, od, sure = expected
    gi, gd = res.indices.cpu().numpy(), res.distances.cpu().numpy()
    assert gi.shape == oi.shape
    assert np.array_equal(gd, od)  # distances bit for bit (every row: a left-out last entry is compared by distance alone)
    assert np.array_equal(gi[:, :-1], oi[:, :-1])
    assert np.array_equal(gi[sure, -1], oi[sure, -1])


# ------------------------------------------------------------------------------------------------------------------ parity

@pytest.mark.parametrize("k", [1, 10, 20, 21, 32, 33, 64, 65, 100])
def test_parity_on_the_reference_cloud(sp, orc, k):
    # 64 / 65: the step from one list entry per lane to two
    tgt, qry = reference_cloud(orc)
    tree = sp.Octree.build(dev(tgt), 0.1, 32)
    assert_rows(tree.knn_search(dev(qry), k), oracle_rows(orc, "reference", tgt, qry, k))


@pytest.mark.parametrize("resolution,max_points", [(100.0, 32), (0.1, 2000), (1e-3, 1), (0.1, 8), (0.1, 200)])
def test_parity_across_structure_parameters(sp, orc, resolution, max_points):
    # (100, 32): the root cell is the cloud's box widened by resolution / 2 per side, so its edge always exceeds the resolution
    # and the root splits once, into leaves of about 125 points; (0.1, 2000): the root alone, one 1000-point leaf — both scanned
    # in 64-point chunks; (1e-3, 1): the deepest tree
    tgt, qry = reference_cloud(orc)
    tree = sp.Octree.build(dev(tgt), resolution, max_points)
    if resolution == 100.0 or max_points == 2000:
        alone = max_points == 2000
        assert tree.info("nodes") == (1 if alone else 9) and tree.info("leaves") == (1 if alone else 8)
        assert tree.info("depth") == (0 if alone else 1)
    for k in (5, 40):
        assert_rows(tree.knn_search(dev(qry), k), oracle_rows(orc, "reference", tgt, qry, k))


@pytest.mark.parametrize("k", [20, 100])
def test_parity_on_nonuniform_density(sp, orc, k):
    tgt, qry = dense_cloud()
    tree = sp.Octree.build(dev(tgt), 0.1, 32)
    assert_rows(tree.knn_search(dev(qry), k), oracle_rows(orc, "nonuniform", tgt, qry, k))


# ------------------------------------------------------------------------------------------------------------------- edges

def bruteforce_equal(orc, tree, qry, tgt, k, T=None):
    r = tree.knn_search(dev(qry), k, T)
    bi, bd = orc.knn_bruteforce(qry if T is None else orc.transform_points(qry, T), tgt, k)
    return np.array_equal(r.indices.cpu().numpy(), bi) and np.array_equal(r.distances.cpu().numpy(), bd)


def test_edges_small_trees(sp, orc):
    g = orc.rng(99)
    qry = g.uniform_points(67, 10.0)
    # n = 0
    empty = sp.Octree.build(dev(np.zeros((0, 4), np.float32)), 0.1)
    r = empty.knn_search(dev(qry), 3)
    assert r.indices.shape == (67, 3) and (r.indices == -1).all() and (r.distances == float(FLT_MAX)).all()
    assert empty.size() == 0 and empty.info("nodes") == 0 and empty.info("next_id") == 0
    # n = 1
    one = sp.Octree.build(dev(np.array([[0, 0, 0, 1]], np.float32)), 0.1)
    r = one.knn_search(dev(np.array([[1, 1, 1, 1]], np.float32)), 3)
    assert r.indices.cpu().numpy().tolist() == [[0, -1, -1]]
    assert r.distances.cpu().numpy().tolist() == [[3.0, float(FLT_MAX), float(FLT_MAX)]]
    # fewer points than k
    five = g.uniform_points(5, 10.0)
    r = sp.Octree.build(dev(five), 0.1).knn_search(dev(qry), 20)
    bi, bd = orc.knn_bruteforce(qry, five, 5)
    gi, gd = r.indices.cpu().numpy(), r.distances.cpu().numpy()
    assert np.array_equal(gi[:, :5], bi) and np.array_equal(gd[:, :5], bd)
    assert (gi[:, 5:] == -1).all() and (gd[:, 5:] == FLT_MAX).all()
    # the first split: 32 points are one leaf, 33 are not
    for n in (32, 33):
        pts = g.uniform_points(n, 10.0)
        tree = sp.Octree.build(dev(pts), 0.1, 32)
        assert (tree.info("nodes") == 1) == (n == 32)
        assert bruteforce_equal(orc, tree, qry, pts, 20)


def test_edges_duplicates_nonfinite_far_queries_and_transform(sp, orc):
    g = orc.rng(5)
    pts = g.uniform_points(3000, 4.0)
    pts[1000:1200] = pts[17]  # 200 exact copies of one point: an over-full leaf at the depth cap, ties to the lowest index
    tree = sp.Octree.build(dev(pts), 0.0, 32)
    nodes, ids = tree.export()
    over = (nodes[:, 6] == 1) & (nodes[:, 9] > 32)
    assert over.sum() == 1 and nodes[over, 7][0] == 21 and nodes[over, 9][0] == 201
    for nq in (1, 67, 257):
        q = g.uniform_points(nq, 4.5)
        q[0] = pts[17]
        assert bruteforce_equal(orc, tree, q, pts, 20)
    dup = tree.knn_search(dev(pts[17:18]), 20).indices.cpu().numpy()[0]
    assert dup.tolist() == [17] + list(range(1000, 1019))
    # one inf and one NaN coordinate among the targets, one NaN query
    bad = pts.copy()
    bad[7, 0] = np.inf
    bad[9, 1] = np.nan
    q = g.uniform_points(67, 4.5)
    q[3, 2] = np.nan
    tree = sp.Octree.build(dev(bad), 0.1, 32)
    assert tree.size() == 2998 and tree.info("next_id") == 3000
    assert bruteforce_equal(orc, tree, q, bad, 20)
    r = tree.knn_search(dev(q), 7)
    assert (r.indices[3] == -1).all() and (r.distances[3] == float(FLT_MAX)).all()
    # queries far outside the box
    far = g.uniform_points(67, 4.0) + np.array([300.0, -2000.0, 50.0, 0.0], np.float32)
    assert bruteforce_equal(orc, tree, far, bad, 20)
    # a transform: the rows of searching T * q
    T = orc.se3_exp(np.array([0.1, -0.2, 0.05, 0.3, -0.1, 0.2], np.float32))
    assert bruteforce_equal(orc, tree, q, bad, 5, T)
    a, b = tree.knn_search(dev(q), 5, T), tree.knn_search(dev(q), 5, dev(np.ascontiguousarray(T.T).reshape(-1)))
    assert torch.equal(a.indices, b.indices) and torch.equal(a.distances, b.distances)  # the matrix in device memory


def test_edges_k_and_repeatability(sp, orc):
    tgt, qry = reference_cloud(orc)
    tree = sp.Octree.build(dev(tgt), 0.1, 32)
    r = tree.knn_search(dev(qry), 0)
    assert tuple(r.indices.shape) == (100, 0) and tuple(r.distances.shape) == (100, 0) and (r.query_size, r.k) == (100, 0)
    with pytest.raises(sp.SpError, match="exceeds the supported maximum"):
        tree.knn_search(dev(qry), 101)
    import sycl_points_amd._lib as _lib
    out_i, out_d = torch.zeros((100, 101), dtype=torch.int32, device="cuda"), torch.zeros((100, 101), device="cuda")
    q = dev(qry)
    rc = _lib.lib().sp_octree_search(tree._h, C.c_void_p(q.data_ptr()), 100, 101, None, 0, C.c_void_p(out_i.data_ptr()),
                                     C.c_void_p(out_d.data_ptr()), None)
    assert rc == _lib.SP_ERR_INVALID_ARGUMENT and (out_i == 0).all()
    for k in (20, 100):
        a, b = tree.knn_search(dev(qry), k), tree.knn_search(dev(qry), k)
        assert a.indices.cpu().numpy().tobytes() == b.indices.cpu().numpy().tobytes()
        assert a.distances.cpu().numpy().tobytes() == b.distances.cpu().numpy().tobytes()


# --------------------------------------------------------------------------------------------------------------- structure

def check_structure(tree, pts, resolution, max_points):
    nodes, ids = tree.export()
    n_nodes = len(nodes)
    box = np.ascontiguousarray(nodes[:, :6]).view(np.float32)
    leaf, depth = nodes[:, 6] == 1, nodes[:, 7]
    finite = np.isfinite(pts[:, :3]).all(1)
    # every finite point id in exactly one leaf: the leaves' slot ranges tile [0, slots), the slots hold each id once
    start, count = nodes[leaf, 8], nodes[leaf, 9]
    order = np.argsort(start)
    assert (count > 0).all() and start[order][0] == 0
    assert np.array_equal(start[order][1:], (start[order] + count[order])[:-1]) and (start + count).max() == len(ids)
    assert np.array_equal(np.sort(ids), np.flatnonzero(finite))
    # a leaf's points inside its box, exactly
    owner = np.empty(len(ids), np.int64)
    for j in np.flatnonzero(leaf):
        owner[nodes[j, 8]:nodes[j, 8] + nodes[j, 9]] = j
    p = pts[ids, :3]
    assert (p >= box[owner, :3]).all() and (p <= box[owner, 3:]).all()
    # children: index above the parent's, one level deeper, box inside the parent's, every node but the root some node's child
    parent = np.full(n_nodes, -1)
    below = np.where(leaf, nodes[:, 9], 0).astype(np.int64)  # points below a node
    for j in np.flatnonzero(~leaf):
        ch = nodes[j, 8:16]
        ch = ch[ch >= 0]
        assert len(ch) >= 1 and (ch > j).all() and (ch < n_nodes).all() and (parent[ch] == -1).all()
        parent[ch] = j
        assert (depth[ch] == depth[j] + 1).all()
        assert (box[ch, :3] >= box[j, :3]).all() and (box[ch, 3:] <= box[j, 3:]).all()
    assert parent[0] == -1 and (parent[1:] >= 0).all() and depth[0] == 0
    for j in range(n_nodes - 1, 0, -1):  # (children come after their parents: a node is complete before it is added)
        below[parent[j]] += below[j]
    assert below[0] == len(ids)
    # the split rule (octree.hpp:416-418, depth cap 21): the root cell is the points' box widened by max(1e-5, resolution / 2),
    # a cell's longest edge is the root's / 2^depth, in float arithmetic
    res = np.float32(resolution)
    eps = max(np.float32(1e-5), res * np.float32(0.5))
    lo = pts[finite, :3].min(0) - eps
    hi = pts[finite, :3].max(0) + eps
    edge = np.ldexp((hi - lo).max().astype(np.float32), -depth.astype(np.int32)).astype(np.float32)
    may_split = (edge > res) & (depth < 21)
    assert not (leaf & (below > max_points) & may_split).any()   # an over-full leaf only where it may not split
    assert ((below > max_points) & may_split)[~leaf].all()       # and nothing split that should not have
    assert tree.info("nodes") == n_nodes and tree.info("leaves") == leaf.sum() and tree.info("depth") == depth.max()
    assert tree.info("next_id") == len(pts) and tree.info("slots") == len(ids) and tree.size() == finite.sum()


@pytest.mark.parametrize("resolution,max_points", [(0.1, 32), (100.0, 32), (0.1, 2000), (1e-3, 1), (0.1, 8), (0.1, 200)])
def test_structure_of_the_reference_cloud(sp, orc, resolution, max_points):
    tgt, _ = reference_cloud(orc)
    check_structure(sp.Octree.build(dev(tgt), resolution, max_points), tgt, resolution, max_points)


def test_structure_of_the_nonuniform_cloud(sp):
    tgt, _ = dense_cloud()
    check_structure(sp.Octree.build(dev(tgt), 0.1, 32), tgt, 0.1, 32)


# ----------------------------------------------------------------------------------------------------------------- removal

def test_removal(sp, orc):
    pts = orc.rng(2025).uniform_points(1024, 10.0)
    tree = sp.Octree.build(dev(pts), 0.1, 32)
    flags = np.ones(1024, np.uint8)
    flags[::7] = 0
    new = np.where(flags == 1, np.cumsum(flags) - 1, -1).astype(np.int32)
    kept = np.ascontiguousarray(pts[flags == 1])
    with pytest.raises(sp.SpError, match="must match the octree point identifier range"):
        tree.remove_nodes_by_flags(dev(flags[:-1]), dev(new[:-1]))
    with pytest.raises(sp.SpError, match="must have the same size"):
        tree.remove_nodes_by_flags(dev(flags), dev(new[:-1]))
    tree.remove_nodes_by_flags(dev(flags), dev(new))
    assert tree.size() == len(kept) == 877 and tree.info("next_id") == 877
    assert bruteforce_equal(orc, tree, kept, kept, 10)
    # a second removal is sized to the new id range
    with pytest.raises(sp.SpError, match="must match the octree point identifier range"):
        tree.remove_nodes_by_flags(dev(flags), dev(new))
    flags2 = np.ones(877, np.uint8)
    flags2[::3] = 0
    new2 = np.where(flags2 == 1, np.cumsum(flags2) - 1, -1).astype(np.int32)
    # a new id at or above n_flags is refused
    wrong = new2.copy()
    wrong[1] = 877
    with pytest.raises(sp.SpError, match="exceeds the allocated range"):
        sp.Octree.build(dev(kept), 0.1, 32).remove_nodes_by_flags(dev(flags2), dev(wrong))
    tree.remove_nodes_by_flags(dev(flags2), dev(new2))
    kept2 = np.ascontiguousarray(kept[flags2 == 1])
    assert tree.size() == len(kept2) and tree.info("next_id") == len(kept2)
    assert bruteforce_equal(orc, tree, kept2, kept2, 10)
    # a flag that is neither 0 nor 1 removes, a negative new index removes, the others are relabelled in reverse
    m = len(kept2)
    flags3 = np.ones(m, np.uint8)
    flags3[0] = 2
    new3 = (m - 1 - np.arange(m)).astype(np.int32)
    new3[1] = -1
    tree.remove_nodes_by_flags(dev(flags3), dev(new3))
    assert tree.size() == m - 2 and tree.info("next_id") == m - 2
    relabelled = np.ascontiguousarray(kept2[2:][::-1])
    assert bruteforce_equal(orc, tree, relabelled, relabelled, 10)
    # a sparse relabelling: the id range follows the largest new id (octree.hpp:368-379)
    sparse = sp.Octree.build(dev(pts[:10]), 0.1, 32)
    f = np.zeros(10, np.uint8)
    f[[2, 4, 6]] = 1
    ni = np.full(10, -1, np.int32)
    ni[[2, 4, 6]] = [9, 0, 5]
    sparse.remove_nodes_by_flags(dev(f), dev(ni))
    assert sparse.size() == 3 and sparse.info("next_id") == 10
    r = sparse.knn_search(dev(pts[[4, 6, 2]]), 3)
    assert r.indices[:, 0].cpu().numpy().tolist() == [0, 5, 9] and (r.distances[:, 0] == 0).all()
    # removing everything: the empty tree
    n3 = tree.info("next_id")
    tree.remove_nodes_by_flags(dev(np.zeros(n3, np.uint8)), dev(np.full(n3, -1, np.int32)))
    assert tree.size() == 0 and tree.info("next_id") == 0
    r = tree.knn_search(dev(kept2[:67]), 4)
    assert (r.indices == -1).all() and (r.distances == float(FLT_MAX)).all()


# --------------------------------------------------------------------------------------------------- report and C++ facade

def test_no_kernel_spills_or_uses_scratch():
    report = os.path.join(ROOT, "sycl_points_amd", "lib", "octree.resources.txt")
    rows = [l for l in open(report) if "Function Name" in l]
    names = " ".join(rows)
    assert "octree_search_kernelILb0E" in names and "octree_search_kernelILb1E" in names and len(rows) >= 12
    for row in rows:
        assert int(re.search(r"VGPRs Spill: (\d+)", row).group(1)) == 0, row
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", row).group(1)) == 0, row


def test_cpp_facade(sp):
    """tests/cpp/test_octree.cpp, built with tests/cpp/Makefile's flags and libraries (the Makefile is not changed): knn::Octree through
    the reference's include path — a search against knn_search_bruteforce, the every-7th removal, the exceptions, and
    Registration::align through the KNNBase seam against the same call with a KDTree; test_octree_header.cpp: the header alone."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(cpp, "test_octree")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.join(ROOT, "sycl_points_amd", "lib")
    flags = ["-std=c++20", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{rocm}/include", "-D__HIP_PLATFORM_AMD__", "-Wall",
             "-Wno-unused-value", "-Wno-unused-result"]
    subprocess.check_call(["g++", "-fsyntax-only", *flags, os.path.join(cpp, "test_octree_header.cpp")])
    subprocess.check_call(["g++", "-O2", *flags, os.path.join(cpp, "test_octree.cpp"), "-o", exe, f"-L{libdir}", "-lsycl_points_amd",
                           f"-Wl,-rpath,{libdir}", f"-L{rocm}/lib", "-lamdhip64", f"-Wl,-rpath,{rocm}/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failed" in r.stdout
