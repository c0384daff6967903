"""Scan Context place recognition on the device (csrc/place_recognition.hip) against tests/f64_scan_context.py.

  1. Descriptor: the device's bits equal the host twin's on every case of the CPU test, and for an empty cloud.
  2. Known shifts: a descriptor rolled by s columns, searched against itself, returns shift s at a distance <= tol, for
     s in {0, 1, h - 1, h, sectors - 1} and the four (rings, sectors) shapes (odd ring counts exercise the zero padding). With
     rings == 1 the definition cannot tell shifts apart (every non-empty column normalises to 1, so d_s == 0 wherever columns
     overlap): there the distance is held to tol and the shift to the lowest shift at which the model's distance is 0.
  3. The search against the float64 model with tol = 2 (rings + sectors + 8) 2^-24 (the 3 roundings of each normalised operand, the
     dot product over the rings, the diagonal sum over the sectors, the divide and the subtract, doubled): every returned distance
     within tol of the model's d_shift of that entry; the model's minimum over shifts not more than tol below it; no entry left
     out whose model distance is below the largest returned one minus 2 tol; rows ascending by (bits of distance, index). Sizes
     N = 0, 1, 2, 63, 64, 65, 1000 with k = 1, 5, 32; sub-ranges; an all-zero query; duplicates; growth from capacity 2.
  4. Two runs of compute, add and search give the same bytes.
  5. End to end: the database holds random, scaled, the bundled target, mirrored; the query is the bundled source turned by 150
     degrees. Candidate 0 is the target at shift 25; its 5 guesses through align_batch and best_of end within twice the errors of
     align_batch started at the truth, while align from the identity ends more than 1 rad off.
  6. The C++ facade (tests/cpp/test_place_recognition.cpp) reproduces the mirror's descriptor bytes, candidates and guesses.
`pytest -s` prints every figure before it is asserted."""
import ctypes as C
import os

import numpy as np
import pytest

import f64_fpfh as reg_model
import f64_scan_context as model

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FLT_MAX = np.float32(np.finfo(np.float32).max)
CASES = model.descriptor_cases()
SIZES = (0, 1, 2, 63, 64, 65, 1000)


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    from sycl_points_amd import _lib

    _lib.build()
    import sycl_points_amd.api as api

    return api


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def api_params(sp, p):
    return sp.ScanContextParams(p["rings"], p["sectors"], p["max_range"], p["sensor_height"])


def tol_of(p):
    return 2.0 * (p["rings"] + p["sectors"] + 8) * 2.0 ** -24


def host_twin(p, points):
    from sycl_points_amd import _lib

    P = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    out = np.full((p["rings"], p["sectors"]), np.nan, np.float32)
    prm = _lib.ScanContextParams(p["rings"], p["sectors"], p["max_range"], p["sensor_height"])
    assert _lib.lib().sp_scan_context_compute_host(C.byref(prm), P.ctypes.data_as(C.c_void_p), len(P), out.ctypes.data_as(C.c_void_p)) == 0
    return out


# ------------------------------------------------------------------------------------------------------------ 1. descriptor
@pytest.mark.parametrize("name,p,points", CASES, ids=[c[0] for c in CASES])
def test_descriptor_equals_the_host_twin(sp, name, p, points):
    got = sp.scan_context(dev(points), api_params(sp, p)).cpu().numpy()
    want = host_twin(p, points)
    diff = got.view(np.uint32) != want.view(np.uint32)
    print(f"\n[scan context {name}] {len(points)} points, {int((want > 0).sum())} of {want.size} bins occupied, {int(diff.sum())} bins differ")
    assert got.shape == want.shape and not diff.any(), np.argwhere(diff)[:5]


def test_descriptor_of_an_empty_cloud(sp):
    for rings, sectors in model.SHAPES:
        got = sp.scan_context(torch.empty((0, 4), dtype=torch.float32, device="cuda"), sp.ScanContextParams(rings, sectors))
        assert got.shape == (rings, sectors) and not got.any()


# ---------------------------------------------------------------------------------------------------------- 2. known shifts
def height_image(rings, sectors, seed, fill=0.35, empty_columns=()):
    """A random descriptor: a share `fill` of the bins occupied, heights in (0, 12]; some columns empty."""
    rs = np.random.RandomState(seed)
    D = (rs.uniform(0.05, 12.0, (rings, sectors)) * (rs.uniform(size=(rings, sectors)) < fill)).astype(np.float32)
    for j in empty_columns:
        D[:, j % sectors] = 0
    return D


def search(db, Q, k, first=0, count=None):
    idx, dist, shift = db.search(dev(Q), k, first, count)
    return idx.cpu().numpy(), dist.cpu().numpy(), shift.cpu().numpy()


@pytest.mark.parametrize("rings,sectors", model.SHAPES)
def test_known_shifts(sp, rings, sectors):
    p = model.params(rings, sectors)
    D = height_image(rings, sectors, 10 * rings + sectors, fill=0.6, empty_columns=(1,))
    if rings == 1:  # one ring: every non-empty column normalises to 1, so only a single non-empty column tells the shifts apart
        D = np.zeros((1, sectors), np.float32)
        D[0, 2] = 3.5
    db = sp.ScanContextDatabase(api_params(sp, p))
    db.add(dev(D))
    h = sectors // 2
    for s in sorted({0, 1, h - 1, h, sectors - 1}):
        Q = np.roll(D, s, axis=1)
        idx, dist, shift = search(db, Q, 1)
        print(f"\n[known shift {rings}x{sectors}] s {s}: index {idx[0]} shift {shift[0]} distance {dist[0]:.3e} (tol {tol_of(p):.3e})", end="")
        zero = np.nonzero(model.shift_distances(Q, D) <= 2 * tol_of(p))[0]
        assert zero.tolist() == [s]  # the rolled shift is the model's only minimiser
        assert idx[0] == 0 and shift[0] == s and 0.0 <= dist[0] <= tol_of(p)


# ------------------------------------------------------------------------------------------------------- 3. against the model
@pytest.fixture(scope="module")
def world():
    """1000 default-shaped descriptors and a query related to some of them; the model's d_s for every entry, computed once."""
    p = model.params()
    entries = [height_image(20, 60, 1000 + i, fill=0.2 + 0.3 * ((i * 7) % 10) / 10, empty_columns=(i, i + 5) if i % 3 == 0 else ())
               for i in range(1000)]
    rs = np.random.RandomState(5)
    base = entries[0].copy()
    for i, s in ((1, 3), (40, 59), (63, 30), (64, 0), (500, 17), (999, 44)):  # noisy turned copies of entry 0
        noisy = base * (1 + rs.normal(0, 0.05 + 0.0002 * i, base.shape)) * (rs.uniform(size=base.shape) < 0.9)
        entries[i] = np.roll(noisy, -s, axis=1).astype(np.float32)
    query = (base * (1 + rs.normal(0, 0.03, base.shape))).astype(np.float32)
    d = np.stack([model.shift_distances(query, e) for e in entries])
    return dict(p=p, entries=entries, query=query, d=d)


@pytest.fixture(scope="module")
def databases(sp, world):
    out = {}
    for n in SIZES:
        db = sp.ScanContextDatabase(api_params(sp, world["p"]), capacity_hint=n)
        for e in world["entries"][:n]:
            db.add(dev(e))
        assert db.size() == n == len(db)
        out[n] = db
    return out


def check_rows(tag, p, d, idx, dist, shift, first, count, k):
    """d: the model's (entries, sectors) distances, rows by ABSOLUTE index"""
    tol = tol_of(p)
    valid = min(k, count)
    assert len(idx) == len(dist) == len(shift) == k
    assert (idx[valid:] == -1).all() and (dist[valid:] == FLT_MAX).all() and (shift[valid:] == 0).all()
    idx, dist, shift = idx[:valid].astype(np.int64), dist[:valid].astype(np.float64), shift[:valid]
    if valid == 0:
        return
    assert ((idx >= first) & (idx < first + count)).all() and len(np.unique(idx)) == valid
    assert ((shift >= 0) & (shift < p["sectors"])).all()
    at_shift, dmin = d[idx, shift], d.min(1)
    err = np.abs(dist - at_shift).max()
    below = (dist - dmin[idx]).max()
    out = np.setdiff1d(np.arange(first, first + count), idx)
    margin = (dmin[out].min() - dmin[idx].max()) if len(out) else np.inf
    keys = (dist.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    print(f"\n[search {tag}] k {k}: |d - model| <= {err:.2e}, d - model minimum <= {below:.2e}, nearest entry left out "
          f"{margin:+.2e} from the farthest returned (tol {tol:.2e})", end="")
    assert err <= tol
    assert below <= tol
    assert margin >= -2 * tol
    assert (keys[1:] > keys[:-1]).all()


@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("n", SIZES)
def test_search_against_the_model(world, databases, n, k):
    idx, dist, shift = search(databases[n], world["query"], k)
    check_rows(f"N {n}", world["p"], world["d"], idx, dist, shift, 0, n, k)
    copies = {0: 0, 1: 3, 40: 59, 63: 30, 64: 0, 500: 17, 999: 44}  # the turned copies of entry 0 come back at their shifts
    assert all(copies[i] == s for i, s in zip(idx.tolist(), shift.tolist()) if i in copies)
    if n == 65 and k >= 5:
        assert set(idx[:5].tolist()) == {0, 1, 40, 63, 64}


@pytest.mark.parametrize("first,count", [(0, 0), (10, 0), (1000, 0), (5, 1), (100, 64), (937, 63), (1, 999), (36, 5)])
def test_search_sub_ranges(world, databases, first, count):
    for k in (1, 32):
        idx, dist, shift = search(databases[1000], world["query"], k, first, count)
        check_rows(f"[{first}, {first + count})", world["p"], world["d"], idx, dist, shift, first, count, k)


@pytest.mark.parametrize("rings,sectors", [(7, 30), (32, 64), (1, 4)])
def test_search_other_shapes(sp, rings, sectors):
    p = model.params(rings, sectors)
    entries = [height_image(rings, sectors, 77 * rings + i, fill=0.5, empty_columns=(i,) if i % 4 == 0 else ()) for i in range(70)]
    query = np.roll(entries[33], 2, axis=1) * np.float32(1.5)  # (a scale does not change a normalised column)
    if rings == 1:  # (entry 33 of this shape is empty; two non-empty columns meet the entries' masks at different shifts)
        query = np.array([[2.0, 0.0, 0.0, 5.0]], np.float32)
    d = np.stack([model.shift_distances(query, e) for e in entries])
    db = sp.ScanContextDatabase(api_params(sp, p))
    for e in entries:
        db.add(dev(e))
    for k in (1, 32):
        idx, dist, shift = search(db, query, k)
        check_rows(f"{rings}x{sectors}", p, d, idx, dist, shift, 0, 70, k)
    if rings > 1:
        assert idx[0] == 33 and shift[0] == 2
    else:  # one ring: the distances are exactly 0 or 1 on both sides, so every returned shift is the model's lowest minimiser
        assert np.array_equal(dist, d.min(1)[idx]) and np.array_equal(shift, d.argmin(1)[idx])
        assert len(set(shift.tolist())) > 1  # (the entries' masks put the first overlap at different shifts)


def test_all_zero_query(world, databases):
    zero = np.zeros((20, 60), np.float32)
    for n in (2, 65, 1000):
        idx, dist, shift = search(databases[n], zero, 32)
        v = min(n, 32)
        assert np.array_equal(idx[:v], np.arange(v)) and (dist[:v] == 1.0).all() and (shift[:v] == 0).all()
        assert (idx[v:] == -1).all() and (dist[v:] == FLT_MAX).all()


def test_duplicates_go_to_the_lower_index(sp):
    p = model.params()
    A, B = height_image(20, 60, 1), height_image(20, 60, 2)
    db = sp.ScanContextDatabase(api_params(sp, p))
    for e in (A, B, A, A, B):
        db.add(dev(e))
    idx, dist, shift = search(db, np.roll(A, 9, axis=1), 5)
    assert idx.tolist() == [0, 2, 3, 1, 4] and shift[:3].tolist() == [9, 9, 9]
    assert dist[0] == dist[1] == dist[2] <= tol_of(p) and dist[3] == dist[4] > 0.3


def test_growth_keeps_the_entries(sp, world):
    small = sp.ScanContextDatabase(api_params(sp, world["p"]), capacity_hint=2)
    large = sp.ScanContextDatabase(api_params(sp, world["p"]), capacity_hint=1024)
    for e in world["entries"][:65]:
        small.add(dev(e))
        large.add(dev(e))
    a, b = search(small, world["query"], 32), search(large, world["query"], 32)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    check_rows("grown", world["p"], world["d"], *a, 0, 65, 32)
    small.clear()
    assert small.size() == 0 and search(small, world["query"], 3)[0].tolist() == [-1, -1, -1]
    small.add(dev(world["entries"][7]))
    idx, dist, shift = search(small, world["query"], 3)
    assert idx.tolist() == [0, -1, -1] and abs(dist[0] - world["d"][7, shift[0]]) <= tol_of(world["p"])


def test_vector_unit_form_of_the_search(sp, world, databases):
    """The A/B form of DESIGN 4.21 (csrc/sp_internal.h: sp_internal_scan_context_search_form(1), products on the vector unit) is
    held to the same model and tolerance, on the default shape and on the three others."""
    from sycl_points_amd import _lib

    L = _lib.lib()
    assert L.sp_internal_scan_context_search_form(7) == -1
    assert L.sp_internal_scan_context_search_form(1) == 0
    try:
        for k in (1, 32):
            idx, dist, shift = search(databases[1000], world["query"], k)
            check_rows("vector unit, N 1000", world["p"], world["d"], idx, dist, shift, 0, 1000, k)
            idx, dist, shift = search(databases[65], world["query"], k, 3, 61)
            check_rows("vector unit, [3, 64)", world["p"], world["d"], idx, dist, shift, 3, 61, k)
        for rings, sectors in ((7, 30), (32, 64), (1, 4)):
            p = model.params(rings, sectors)
            entries = [height_image(rings, sectors, 31 * rings + i, fill=0.5, empty_columns=(i,) if i % 4 == 0 else ()) for i in range(70)]
            query = np.roll(entries[12], 3, axis=1)
            d = np.stack([model.shift_distances(query, e) for e in entries])
            db = sp.ScanContextDatabase(api_params(sp, p))
            for e in entries:
                db.add(dev(e))
            idx, dist, shift = search(db, query, 32)
            check_rows(f"vector unit, {rings}x{sectors}", p, d, idx, dist, shift, 0, 70, 32)
            assert rings == 1 or (idx[0] == 12 and shift[0] == 3)
    finally:
        assert L.sp_internal_scan_context_search_form(0) == 1


# --------------------------------------------------------------------------------------------------------- 4. reproducible
def test_two_runs_give_the_same_bytes(sp, world):
    pts = dev(model.scan(40000, 3))
    runs = []
    for _ in range(2):
        D = sp.scan_context(pts)
        db = sp.ScanContextDatabase(capacity_hint=4)
        for e in world["entries"][:200]:
            db.add(dev(e))
        db.add(D)
        out = db.search(D, 32)
        runs.append(b"".join(t.cpu().numpy().tobytes() for t in (D,) + tuple(out)))
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------------------------ 5. end to end
@pytest.fixture(scope="module")
def loop(sp):
    """The four entries, the query, and the database of the end-to-end case."""
    query, entries = model.bundled_clouds(GOLD)
    db = sp.ScanContextDatabase()
    for e in entries:
        db.add(sp.PointCloudShared(dev(e)))
    D = sp.scan_context(sp.PointCloudShared(dev(query)))
    return dict(db=db, D=D, query=query, entries=entries, candidates=db.query(D, 4))


def prepared(sp, name, turn):
    """tests/test_gpu_global_registration.py's preparation: box filter, 1 m voxels, the turn about the sensor, 20-NN covariances"""
    pts = dev(model.read_ply_xyz(os.path.join(GOLD, name + ".ply")))
    pts = sp.compact_by_flags(pts, sp.box_filter_flags(pts, 0.5, 50.0)).contiguous()
    xyz = sp.VoxelGrid(1.0).downsampling(sp.PointCloudShared(pts)).points.contiguous().cpu().numpy()
    if turn is not None:
        xyz[:, :3] = (xyz[:, :3].astype(np.float64) @ turn[:3, :3].T).astype(np.float32)
    xyz[:, 3] = 1.0
    c = sp.PointCloudShared(dev(xyz))
    tree = sp.KDTree.build(c.points)
    sp.covariance.estimate(tree.knn_search(c, 20), c)
    return c, tree


def registration(sp):
    return sp.Registration(sp.RegistrationParams(reg_type="GICP", max_correspondence_distance=2.0, max_iterations=30))


def test_end_to_end_loop_closure(sp, loop):
    cands = loop["candidates"]
    found = [(c.index, round(c.distance, 4), c.shift) for c in cands]
    print(f"\n[loop closure] candidates (index, distance, shift): {found}", end="")
    assert len(cands) == 4 and cands[0].index == 2 and cands[0].shift == 25
    assert abs(cands[0].yaw - np.radians(150.0)) < 1e-6 and cands[0].sectors == 60
    p = model.params()
    want = [model.distance(model.descriptor(loop["query"], p), model.descriptor(e, p))[0] for e in loop["entries"]]
    for c in cands:
        assert abs(c.distance - want[c.index]) <= tol_of(p), (c, want)
    # the alignment the candidate's guesses make possible
    Rz = reg_model.rot_z(150.0)
    T_true = np.loadtxt(os.path.join(GOLD, "T_target_source.txt")) @ np.linalg.inv(Rz)
    S, _ = prepared(sp, "source", Rz)
    Tg, tree = prepared(sp, "target", None)
    start = registration(sp).align(S, Tg, tree)
    st, sr = reg_model.pose_errors(start.T, T_true)
    prep = sp.PreparedTarget(sp.GridKNN.build(Tg.points), Tg.covs)
    ref = registration(sp).align_batch(S, prep, [T_true.astype(np.float32)])[0]
    rt, rr = reg_model.pose_errors(ref.T, T_true)
    guesses = sp.scan_context_guesses(cands[0], 5)
    reg = registration(sp)
    results = reg.align_batch(S, prep, guesses)
    best = reg.best_of(results)
    assert best < len(results)
    gt, gr = reg_model.pose_errors(results[best].T, T_true)
    print(f" | align from the identity ends {st:.2f} m, {sr:.3f} rad off | align_batch from the truth {rt:.3e} m {rr:.3e} rad | from the "
          f"5 guesses (best: {best}, {results[best].inlier} inliers) {gt:.3e} m {gr:.3e} rad")
    assert sr > 1.0  # the need
    assert len(guesses) == 5 and np.allclose(guesses[2], np.linalg.inv(Rz), atol=1e-6)
    assert gt <= 2.0 * rt and gr <= 2.0 * rr, ((gt, gr), (rt, rr))


# ------------------------------------------------------------------------------------------------------- 6. the C++ facade
def fnv1a64(raw):
    h = 1469598103934665603
    for byte in raw:
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_facade(sp, loop, tmp_path):
    """place_recognition::ScanContext, ScanContextDatabase and initial_guesses of the C++ facade (tests/cpp/
    test_place_recognition.cpp, built here with the facade tests' flags) on the end-to-end case's clouds: the descriptor bytes,
    the candidates and the guesses are the Python mirror's, bit for bit."""
    import subprocess

    from test_gpu_lidar_odometry import build

    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = build(os.path.join(cpp, "test_place_recognition.cpp"), os.path.join(cpp, "test_place_recognition"))
    path = str(tmp_path / "clouds.bin")
    clouds = [loop["query"]] + loop["entries"]
    with open(path, "wb") as f:
        f.write(np.array([len(clouds)] + [len(c) for c in clouds], np.int32).tobytes())
        for c in clouds:
            f.write(np.ascontiguousarray(c, np.float32).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout[-4000:]
    for name in ("descriptors", "database", "guesses"):
        assert f"[  OK  ] {name}" in r.stdout, name
    sums, cands, poses = {}, [], {}
    for line in r.stdout.splitlines():
        w = line.split()
        if line.startswith("F "):
            sums[w[1]] = int(w[2], 16)
        elif line.startswith("C "):
            cands.append((int(w[1]), int(w[2], 16), int(w[3]), int(w[4], 16)))
        elif line.startswith("T "):
            poses[w[1]] = np.array([int(x, 16) for x in w[2:]], np.uint32).view(np.float32).reshape(4, 4).T
    assert sums["query"] == fnv1a64(loop["D"].cpu().numpy().tobytes())
    for i, e in enumerate(loop["entries"]):
        assert sums[f"entry{i}"] == fnv1a64(sp.scan_context(dev(e)).cpu().numpy().tobytes()), i
    bits = lambda x: int(np.float32(x).view(np.uint32))  # noqa: E731
    assert cands == [(c.index, bits(c.distance), c.shift, bits(c.yaw)) for c in loop["candidates"]]
    guesses = sp.scan_context_guesses(loop["candidates"][0], 5)
    for i, T in enumerate(guesses):
        assert poses[f"guess{i}"].tobytes() == T.tobytes(), i



def test_example_loop_closure(sp):
    """examples/example_loop_closure.cpp, built with the facade tests' flags, recognises the bundled target among its decoys and
    aligns to it from the candidate's guesses (its exit code holds the result to 0.2 m and 0.03 in the rotation's Frobenius norm)."""
    import subprocess

    from test_gpu_lidar_odometry import build

    exe = build(os.path.join(ROOT, "examples", "example_loop_closure.cpp"), os.path.join(ROOT, "tests", "cpp", "example_loop_closure"))
    r = subprocess.run([exe, os.path.join(GOLD, "source.ply"), os.path.join(GOLD, "target.ply"), os.path.join(GOLD, "T_target_source.txt")],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "<- the place" in r.stdout and "at shift 25" in r.stdout, r.stdout[-3000:]
