"""OccupancyGridMap on the GPU (sp_ogm_*, api.OccupancyGridMap and, through tests/cpp/test_occupancy_grid.cpp, the C++ facade) against
the CPU restatement (tests/cpp/occupancy_grid_restate.cpp, pinned by tests/test_occupancy_grid_cpu.py, whose helpers are used here).

Rows are aligned by voxel key, never by position. What is exact: the set of keys (the free cells the walk creates included),
hit_count, miss_count, last_updated, voxel_num, capacity, the occupied set. What is not:
  * centroid / rgb / intensity sums are relaxed float atomics (order unspecified, as in the reference): held to the bar of
    tests/test_gpu_voxel_hash_map.py for the same kind of sum, 2e-6 relative to the attribute's scale, on the voxel means;
  * log_odds: within n_updates x ulp(max(|pending|, 4)) of the restatement, the bound of a sum of n_updates terms in any order (the
    device forms it from two integer counts, DESIGN.md 7, so it is in fact the restatement's value);
  * covariances: E_ref = the restatement's largest error against a float64 evaluation of the same formulae on these inputs,
    E_dev the device's; required E_dev <= 4 x E_ref + 1e-6 (the factor covers the order of summation). Both are printed (-s).
Measured figures: none yet (DESIGN.md 4.10 says so until the first session with an MI355X writes them down)."""
import importlib.util
import os
import subprocess
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 4096)  # one lane | a wave and its edges | many workgroups
VOXEL = 0.5
ATTR_SCALE = {"rgb": 1.0, "intensities": 100.0}
SUM_BAR = 2e-6


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


@pytest.fixture(scope="module")
def cpu():
    spec = importlib.util.spec_from_file_location("ogm_cpu_helpers", os.path.join(ROOT, "tests", "test_occupancy_grid_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def R(cpu, tmp_path_factory):
    return cpu.build_restatement(tmp_path_factory.mktemp("ogm_gpu"))


def dev_cloud(sp, pts, covs=None, rgb=None, intensities=None):
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    if len(pts) == 0:
        return sp.PointCloudShared()
    return sp.PointCloudShared(d(pts), covs=d(covs), rgb=d(rgb), intensities=d(intensities))


class DevMap:
    """api.OccupancyGridMap behind the interface of the restatement's RestatedMap"""

    def __init__(self, sp, voxel_size):
        self.sp, self.m = sp, sp.OccupancyGridMap(voxel_size)

    def set(self, name, value):
        self.m._set(name, value)

    def set_log_odds_limits(self, lo, hi):
        self.m.set_log_odds_limits(lo, hi)

    def info(self, name):
        return self.m.info(name)

    def add_point_cloud(self, pts, pose=None, covs=None, rgb=None, intensities=None):
        self.m.add_point_cloud(dev_cloud(self.sp, pts, covs, rgb, intensities), pose)

    def extract_occupied_points(self, pose=None, max_distance=100.0):
        r = self.m.extract_occupied_points(pose, max_distance)
        host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        return {"points": host(r.points).reshape(-1, 4), "covs": host(r.covs) if r.has_cov() else None,
                "rgb": host(r.rgb) if r.has_rgb() else None, "intensities": host(r.intensities) if r.has_intensity() else None,
                "keys": host(r.keys).view(np.uint64)}

    def compute_overlap_ratio(self, pts, pose=None):
        return self.m.compute_overlap_ratio(dev_cloud(self.sp, pts), pose)

    def voxel_probability(self, xyz):
        return self.m.voxel_probability(xyz)

    def export(self):
        return self.m.export()


def pose_of(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T.astype(np.float32)


POSE = pose_of(0.3, -0.2, 0.7, (0.137, -0.211, 0.373))  # not the identity; the sensor sits off the lattice of every voxel size used


def make_cloud(n, seed, extent=8.0):
    rs = np.random.RandomState(seed)
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = rs.uniform(-extent, extent, (n, 3)).astype(np.float32)
    A = rs.normal(0, 0.3, (n, 3, 3)).astype(np.float32)
    covs = np.zeros((n, 4, 4), np.float32)
    covs[:, :3, :3] = A @ A.transpose(0, 2, 1) + 0.02 * np.eye(3, dtype=np.float32)
    return dict(pts=pts, covs=covs.reshape(n, 16), rgb=rs.uniform(0, 1, (n, 4)).astype(np.float32),
                intensities=rs.uniform(0, 100, n).astype(np.float32))


@pytest.fixture(scope="module")
def clouds():
    big = make_cloud(4096, seed=31)
    return {n: {k: v[:n] for k, v in big.items()} for n in SIZES}


def by_key(exp):
    o = np.argsort(exp["keys"], kind="stable")
    return {k: v[o] for k, v in exp.items()}


def ulp(x):
    return np.spacing(np.asarray(x, np.float32))


def compare_state(dev, ref, xyz_scale, log_hit=0.85, log_miss=-0.4):
    """device export against the restatement's; returns the number of voxels"""
    d, r = by_key(dev.export()), by_key(ref.export())
    assert np.array_equal(d["keys"], r["keys"]), (len(d["keys"]), len(r["keys"]))
    assert len(np.unique(d["keys"])) == len(d["keys"])
    assert dev.info("voxel_num") == ref.info("voxel_num") == len(d["keys"])
    assert dev.info("capacity") == ref.info("capacity") and dev.info("frame_index") == ref.info("frame_index")
    for k in ("hit_count", "miss_count", "last_updated"):
        assert np.array_equal(d[k], r[k]), k
    cnt = np.maximum(r["hit_count"], 1).astype(np.float64)
    for name, scale in (("sum_xyz", xyz_scale), ("rgb_sums", ATTR_SCALE["rgb"]), ("intensity_sums", ATTR_SCALE["intensities"])):
        err = np.abs(d[name].astype(np.float64) - r[name]) / (cnt if d[name].ndim == 1 else cnt[:, None])
        assert err.max(initial=0.0) <= SUM_BAR * scale, (name, err.max())
    # log-odds: a sum of n_updates terms of at most max(|pending|, 4) in magnitude (the clamp keeps the running value inside +-4)
    n_upd = r["hit_count"].astype(np.float64) + r["miss_count"]
    pending = np.abs(r["hit_count"].astype(np.float64) * log_hit) + np.abs(r["miss_count"].astype(np.float64) * log_miss)
    bound = n_upd * ulp(np.maximum(pending, 4.0).astype(np.float32))
    assert (np.abs(d["log_odds"].astype(np.float64) - r["log_odds"]) <= bound).all()
    return len(d["keys"])


def compare_occupied(dev, ref, pose, max_distance, thr=0.0):
    """the inputs' conditions on the restatement first (no log-odds within 1e-3 of the threshold, no centroid within 1e-4 of
    max_distance), then the occupied set: exact"""
    e = ref.export()
    seen = e["hit_count"] > 0
    assert (np.abs(e["log_odds"] - thr) > 1e-3).all()
    cen = e["sum_xyz"][seen].astype(np.float64) / e["hit_count"][seen][:, None]
    linf = np.abs(cen - np.asarray(pose, np.float64)[:3, 3]).max(axis=1)
    assert (np.abs(linf - max_distance) > 1e-4).all()
    ro, do = ref.extract_occupied_points(pose, max_distance), dev.extract_occupied_points(pose, max_distance)
    assert np.array_equal(np.sort(do["keys"]), np.sort(ro["keys"])) and len(ro["keys"]) <= int(seen.sum())
    return ro, do


def f64_cov_means(ref, frames):
    """exp(mean over the voxel's hits of log(R C R^T)) in float64, per voxel key, over (cloud, pose) frames"""
    logs, counts = {}, {}
    for c, pose in frames:
        keys = ref.point_keys(c["pts"], pose)
        Rm = np.asarray(pose, np.float64)[:3, :3]
        C3 = c["covs"].reshape(-1, 4, 4).transpose(0, 2, 1)[:, :3, :3].astype(np.float64)
        rot = Rm @ C3 @ Rm.T
        w, V = np.linalg.eigh(rot)
        L = (V * np.log(np.maximum(w, 1e-6))[:, None, :]) @ V.transpose(0, 2, 1)
        for k, l in zip(keys, L):
            logs[k] = logs.get(k, 0) + l
            counts[k] = counts.get(k, 0) + 1
    out = {}
    for k, l in logs.items():
        w, V = np.linalg.eigh(l / counts[k])
        out[k] = (V * np.exp(w)) @ V.T
    return out


def check_covariances(dev, ref, frames, label):
    want = f64_cov_means(ref, frames)
    ro, do = ref.extract_occupied_points(None, 1e6), dev.extract_occupied_points(None, 1e6)
    errs = []
    for out in (ro, do):
        got = out["covs"].reshape(-1, 4, 4).transpose(0, 2, 1)
        assert not got[:, 3, :].any() and not got[:, :, 3].any()
        errs.append(max(np.abs(g[:3, :3] - want[k]).max() for k, g in zip(out["keys"], got)))
    E_ref, E_dev = errs
    print(f"occupancy grid covariances [{label}]: E_dev = {E_dev:.3e}  E_ref = {E_ref:.3e}  bound = 4 x E_ref + 1e-6 = {4 * E_ref + 1e-6:.3e}")
    assert E_dev <= 4 * E_ref + 1e-6, (label, E_dev, E_ref)


def attribute_means(dev, ref, xyz_scale):
    ro, do = ref.extract_occupied_points(None, 1e6), dev.extract_occupied_points(None, 1e6)
    assert np.array_equal(np.sort(do["keys"]), np.sort(ro["keys"]))
    oi, di = np.argsort(ro["keys"]), np.argsort(do["keys"])
    assert np.abs(do["points"][di] - ro["points"][oi]).max() <= SUM_BAR * xyz_scale and (do["points"][:, 3] == 1).all()
    for k, scale in ATTR_SCALE.items():
        assert np.abs(do[k][di] - ro[k][oi]).max() <= SUM_BAR * scale, k


XYZ_SCALE = 16.0  # |map-frame coordinate| of a point within +-8 m of a sensor within 1 m of the origin, rotated: below 8 sqrt(3) + 1


def test_reference_known_answers(sp, cpu):
    cpu.known_answers(lambda vs: DevMap(sp, vs), lambda m, pts, pose=None, covs=None, rgb=None, inten=None:
                      m.add_point_cloud(pts, pose, covs, rgb, inten), lambda m, pose, d: m.extract_occupied_points(pose, d),
                      lambda m, q, pose: m.compute_overlap_ratio(q, pose))
    with pytest.raises(sp.SpError) as e:
        sp.OccupancyGridMap(0.0)
    assert e.value.code == 1
    m = sp.OccupancyGridMap(0.25)
    assert m.voxel_size() == 0.25 and m.get("log_odds_hit") == pytest.approx(0.85) and m.get("log_odds_miss") == pytest.approx(-0.4)
    assert (m.get("log_odds_min"), m.get("log_odds_max"), m.get("occupancy_threshold")) == (-4.0, 4.0, 0.5)
    assert m.get("free_space_updates_enabled") == 1 and m.get("voxel_pruning_enabled") == 1
    assert m.get("stale_frame_threshold") == 100 and m.get("rehash_threshold") == pytest.approx(0.7) and m.info("capacity") == 30029


@pytest.mark.parametrize("n", SIZES)
def test_hits_only(sp, cpu, R, clouds, n):
    c = clouds[n]
    dev, ref = DevMap(sp, VOXEL), cpu.RestatedMap(R, VOXEL)
    for m in (dev, ref):
        m.set("free_space_updates_enabled", 0)
        m.add_point_cloud(c["pts"], POSE, c["covs"], c["rgb"], c["intensities"])
    voxels = compare_state(dev, ref, XYZ_SCALE)
    assert dev.export()["miss_count"].sum() == 0 and dev.export()["hit_count"].sum() == n and voxels <= n
    assert all(dev.info(k) == 1 for k in ("has_cov", "has_rgb", "has_intensity"))
    attribute_means(dev, ref, XYZ_SCALE)
    check_covariances(dev, ref, [(c, POSE)], f"hits only, n = {n}")


@pytest.mark.parametrize("n", SIZES)
def test_carving(sp, cpu, R, clouds, n):
    """rays of at most 8 sqrt(3) = 13.9 m from a sensor off the lattice: at most ~90 steps each"""
    c = clouds[n]
    dev, ref = DevMap(sp, VOXEL), cpu.RestatedMap(R, VOXEL)
    for m in (dev, ref):
        m.add_point_cloud(c["pts"], POSE, c["covs"], c["rgb"], c["intensities"])
    voxels = compare_state(dev, ref, XYZ_SCALE)
    e = dev.export()
    assert e["hit_count"].sum() == n and e["miss_count"].sum() > 5 * n and voxels > n  # the walk created free cells
    only_missed = (e["hit_count"] == 0) & (e["miss_count"] > 0)
    assert only_missed.any()  # their log-odds is the miss count again: max(-4, -0.4 m)
    assert np.allclose(e["log_odds"][only_missed], np.maximum(-4.0, np.float32(-0.4) * e["miss_count"][only_missed]), atol=1e-6)
    ro, _ = compare_occupied(dev, ref, POSE, 6.0)
    if n == 4096:
        assert 0 < len(ro["keys"]) < int((e["hit_count"] > 0).sum())  # the distance bound keeps some and drops some
    attribute_means(dev, ref, XYZ_SCALE)


def test_duplicates_and_contention(sp, cpu, R):
    """4096 copies of one point along +x from the origin: every lane of every wave on the same eleven slots"""
    pts = cpu.P([[5.3, 0.1, 0.1]] * 4096)
    dev, ref = DevMap(sp, VOXEL), cpu.RestatedMap(R, VOXEL)
    for m in (dev, ref):
        m.add_point_cloud(pts)
    compare_state(dev, ref, 6.0)
    e = by_key(dev.export())
    cells = (e["keys"] & np.uint64((1 << 21) - 1)).astype(np.int64) - (1 << 20)
    assert np.array_equal(cells, np.arange(11))  # x cells 0 .. 10, y = z = 0
    assert np.array_equal(e["hit_count"], [0] * 10 + [4096]) and np.array_equal(e["miss_count"], [4096] * 10 + [0])
    assert np.allclose(e["log_odds"], [-4.0] * 10 + [4.0])  # clamped


def test_origin_voxel_rule(sp, cpu, R):
    """a point inside the sensor's own cell: no ray posts a miss to that cell (:1427)"""
    pts = cpu.P([[0.05, 0.02, -0.01], [3.3, 1.2, 0.4], [-2.7, 0.3, 1.9], [0.4, -4.4, 0.2]])
    for with_origin_point in (True, False):
        dev, ref = DevMap(sp, VOXEL), cpu.RestatedMap(R, VOXEL)
        for m in (dev, ref):
            m.add_point_cloud(pts if with_origin_point else pts[1:], POSE)
        compare_state(dev, ref, 8.0)
        e = dev.export()
        origin_key = ref.point_keys(cpu.P([[0, 0, 0]]), POSE)[0]
        row = np.flatnonzero(e["keys"] == origin_key)
        assert len(row) == 1
        assert (e["hit_count"][row[0]], e["miss_count"][row[0]]) == ((1, 0) if with_origin_point else (0, 3))


def test_growth_before_the_walk(sp, cpu, R, clouds):
    """4096 rays at voxel 0.25: the estimated visits exceed 0.7 x 30 029, the table grows before the walk and loses nothing"""
    c = clouds[4096]
    dev, ref = DevMap(sp, 0.25), cpu.RestatedMap(R, 0.25)
    for m in (dev, ref):
        m.add_point_cloud(c["pts"], POSE)
    voxels = compare_state(dev, ref, XYZ_SCALE)
    assert dev.info("capacity") > 30029 and voxels > 0.7 * 30029 and voxels == dev.info("voxel_num")


def test_skipped_rays(sp, cpu, R, clouds):
    """points with NaN or Inf, or 1e7 m away, change nothing and cost nothing; no device error"""
    c = clouds[4096]
    bad = cpu.P([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [1e7, 0, 0], [0, -1e7, 3], [2, 2, 1e7], [np.nan] * 3])
    mixed = np.concatenate([c["pts"][:2048], bad, c["pts"][2048:]])
    times, exports = [], []
    for pts in (c["pts"], mixed, c["pts"], mixed):  # the first of each pays for warm-up
        m = DevMap(sp, VOXEL)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.add_point_cloud(pts, POSE)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        exports.append(by_key(m.export()))
    for k in ("keys", "hit_count", "miss_count", "last_updated", "log_odds"):
        assert np.array_equal(exports[2][k], exports[3][k]), k
    print(f"skipped rays: add_point_cloud {times[2] * 1e3:.2f} ms without, {times[3] * 1e3:.2f} ms with the seven bad points")
    assert times[3] <= times[2] + 0.25  # a walk of 2e7 cells is seconds of probing
    ref = cpu.RestatedMap(R, VOXEL)
    ref.add_point_cloud(mixed, POSE)
    assert np.array_equal(exports[3]["keys"], by_key(ref.export())["keys"])
    far = DevMap(sp, VOXEL)  # a sensor outside the cell range: the hits are invalid too, nothing happens, the frame counts
    far.add_point_cloud(c["pts"][:64], pose_of(0, 0, 0, (1e7, 0, 0)))
    assert far.info("voxel_num") == 0 and far.info("frame_index") == 1


def test_pruning_then_reinsertion(sp, cpu, R):
    """a pruned key comes back into its `deleted` slot"""
    A, B = cpu.P([[0.1, 0.1, 0.1]]), cpu.P([[3.1, 0.1, 0.1]])
    dev, ref = DevMap(sp, VOXEL), cpu.RestatedMap(R, VOXEL)
    for m in (dev, ref):
        m.set("free_space_updates_enabled", 0)
        m.set("stale_frame_threshold", 2)
        m.add_point_cloud(A)
        for _ in range(3):
            m.add_point_cloud(B)
    compare_state(dev, ref, 4.0)
    assert dev.info("voxel_num") == 1 and dev.voxel_probability(A[0, :3]) == 0.5 and dev.voxel_probability(B[0, :3]) > 0.5
    for m in (dev, ref):
        m.add_point_cloud(np.concatenate([A, B]))
    compare_state(dev, ref, 4.0)
    e = by_key(dev.export())
    assert dev.info("voxel_num") == 2 and dev.info("capacity") == 30029
    assert sorted(e["hit_count"].tolist()) == [1, 4] and sorted(e["last_updated"].tolist()) == [4, 4]
    assert dev.voxel_probability(A[0, :3]) == pytest.approx(1 / (1 + np.exp(-0.85)), abs=1e-6)


def test_multi_frame(sp, cpu, R):
    """five frames of 1024 points from a moving sensor, every attribute, carving on: the restatement's state"""
    dev, ref = DevMap(sp, VOXEL), cpu.RestatedMap(R, VOXEL)
    frames = []
    for f in range(5):
        c = make_cloud(1024, seed=100 + f)
        pose = pose_of(0.05 * f, -0.03 * f, 0.2 * f, (0.137 + 0.9 * f, -0.211 + 0.4 * f, 0.373 - 0.2 * f))
        frames.append((c, pose))
        for m in (dev, ref):
            m.add_point_cloud(c["pts"], pose, c["covs"], c["rgb"], c["intensities"])
    compare_state(dev, ref, XYZ_SCALE + 4.0)
    ro, _ = compare_occupied(dev, ref, frames[-1][1], 6.0)
    assert len(ro["keys"]) > 0
    attribute_means(dev, ref, XYZ_SCALE + 4.0)
    check_covariances(dev, ref, frames, "five frames of 1024")
    q = make_cloud(2048, seed=7)["pts"]
    assert dev.compute_overlap_ratio(q, frames[2][1]) == pytest.approx(ref.compute_overlap_ratio(q, frames[2][1]), abs=1e-7)
    for p in q[:32, :3]:
        assert dev.voxel_probability(p) == pytest.approx(ref.voxel_probability(p), abs=1e-6)


def test_empty_and_absent_inputs(sp, cpu, R):
    """:130-132, 176-178, 418-420"""
    m = sp.OccupancyGridMap(VOXEL)
    m.add_point_cloud(sp.PointCloudShared())
    assert m.info("frame_index") == 0 and m.info("voxel_num") == 0
    r = m.extract_occupied_points()
    assert r.size() == 0 and len(r.keys) == 0 and len(m.export()["keys"]) == 0
    q = dev_cloud(sp, cpu.P([[0.1, 0.1, 0.1]]))
    assert m.compute_overlap_ratio(q) == 0.0 and m.voxel_probability([0.1, 0.1, 0.1]) == 0.5
    m.add_point_cloud(q)  # no attributes
    assert m.info("frame_index") == 1 and not (m.info("has_cov") or m.info("has_rgb") or m.info("has_intensity"))
    r = m.extract_occupied_points()
    assert r.size() == 1 and not r.has_cov() and not r.has_rgb() and not r.has_intensity()
    assert m.compute_overlap_ratio(sp.PointCloudShared()) == 0.0 and m.compute_overlap_ratio(q) == 1.0
    m.clear()
    assert m.info("voxel_num") == 0 and m.info("frame_index") == 0 and m.extract_occupied_points().size() == 0


def test_export_scratch_regrows(sp, cpu, R):
    """Two rounds of exports of one map object either side of a rehash: the compaction scratch (flags, positions, scan workspace) is
    sized for 30 029 slots by the first round and has to grow for the 60 013 of the second. Hits only, one point per voxel at the
    cell centres (exact in fp32: no centroid on a box face); rehash_threshold 0.01 grows the table at the first add that finds more
    than 300 voxels: 64 voxels -> exports -> +250 (314) -> +150 (rehash first, then 464) -> exports."""
    dev, ref = DevMap(sp, VOXEL), cpu.RestatedMap(R, VOXEL)
    for m in (dev, ref):
        m.set("free_space_updates_enabled", 0)
        m.set("rehash_threshold", 0.01)
    first = 0
    for frames, voxels, capacity in (((64,), 64, 30029), ((250, 150), 464, 60013)):
        for count in frames:
            k = np.arange(first, first + count)
            first += count
            pts = cpu.P((np.stack([k % 8, (k // 8) % 8, k // 64], axis=1) + 0.5) * VOXEL)
            rgb = np.stack([(k % 7) / 8.0, (k % 5) / 8.0, (k % 3) / 4.0, np.ones(count)], axis=1).astype(np.float32)
            for m in (dev, ref):
                m.add_point_cloud(pts, None, None, rgb, (k % 11).astype(np.float32))
        assert compare_state(dev, ref, 4.0) == voxels  # export(): keys, counts, voxel_num, capacity exact
        assert dev.info("capacity") == capacity
        attribute_means(dev, ref, 4.0)  # extract_occupied_points: the same key set, the means
        assert len(dev.extract_occupied_points(None, 1e6)["keys"]) == voxels  # one hit each: log-odds 0.85, occupied


def test_cpp_facade(sp):
    """tests/cpp/test_occupancy_grid.cpp, built with tests/cpp/Makefile's flags and libraries (the Makefile is not changed): the
    reference's known answers and one carving case through sycl_points::algorithms::mapping::OccupancyGridMap"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(cpp, "test_occupancy_grid")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    lib = os.path.join(ROOT, "sycl_points_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++20", f"-I{ROOT}/include", f"-I{rocm}/include", "-D__HIP_PLATFORM_AMD__", "-Wall",
                           "-Wno-unused-value", "-Wno-unused-result", os.path.join(cpp, "test_occupancy_grid.cpp"), "-o", exe,
                           f"-L{lib}", "-lsycl_points_amd", f"-Wl,-rpath,{lib}", f"-L{rocm}/lib", "-lamdhip64",
                           f"-Wl,-rpath,{rocm}/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failed" in r.stdout
