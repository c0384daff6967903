"""OccupancyGridMap without a device: the CPU restatement (tests/cpp/occupancy_grid_restate.cpp; mapping/occupancy_grid_map.hpp of
the reference, with the bounded ray walk of DESIGN.md 4.10) pinned on the reference's own known answers
(cpp/tests/test_occupancy_grid_map.cpp:90-523, its tolerances: 1e-5, 1e-4 for the rotated covariance), the bounded walk against a
float64 enumeration of the cells a segment crosses, the ray on which an unbounded walk does not end, the C ABI's argument checks
(SP_ERR_INVALID_ARGUMENT before any HIP call) and the compiler's resource report for the walk kernel.
The GPU suite (tests/test_gpu_occupancy_grid.py) holds the device to this restatement; its helpers live here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM = {"voxel_size": 0, "log_odds_hit": 1, "log_odds_miss": 2, "log_odds_min": 3, "log_odds_max": 4, "occupancy_threshold": 5,
         "free_space_updates_enabled": 6, "voxel_pruning_enabled": 7, "stale_frame_threshold": 8, "rehash_threshold": 9}
INFO = {"voxel_num": 0, "capacity": 1, "frame_index": 2, "has_cov": 3, "has_rgb": 4, "has_intensity": 5}
EXPORT_FIELDS = (("keys", np.uint64, ()), ("hit_count", np.uint32, ()), ("miss_count", np.uint32, ()), ("log_odds", np.float32, ()),
                 ("last_updated", np.uint32, ()), ("sum_xyz", np.float32, (3,)), ("cov_sums", np.float32, (6,)),
                 ("rgb_sums", np.float32, (4,)), ("intensity_sums", np.float32, ()))


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libogm_restate.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "occupancy_grid_restate.cpp"), "-o", so])
    R = C.CDLL(so)
    vp, u64, f, i = C.c_void_p, C.c_uint64, C.c_float, C.c_int
    R.ogm_restate_create.restype, R.ogm_restate_create.argtypes = vp, [f]
    R.ogm_restate_destroy.restype, R.ogm_restate_destroy.argtypes = None, [vp]
    R.ogm_restate_clear.restype, R.ogm_restate_clear.argtypes = None, [vp]
    R.ogm_restate_set.restype, R.ogm_restate_set.argtypes = i, [vp, i, f]
    R.ogm_restate_set_limits.restype, R.ogm_restate_set_limits.argtypes = i, [vp, f, f]
    R.ogm_restate_threshold_log_odds.restype, R.ogm_restate_threshold_log_odds.argtypes = f, [vp]
    R.ogm_restate_info.restype, R.ogm_restate_info.argtypes = u64, [vp, i]
    R.ogm_restate_add.restype, R.ogm_restate_add.argtypes = None, [vp, vp, vp, vp, vp, u64, vp]
    R.ogm_restate_extract.restype, R.ogm_restate_extract.argtypes = u64, [vp, vp, f, vp, vp, vp, vp, vp]
    R.ogm_restate_overlap.restype, R.ogm_restate_overlap.argtypes = f, [vp, vp, u64, vp]
    R.ogm_restate_probability.restype, R.ogm_restate_probability.argtypes = f, [vp, vp]
    R.ogm_restate_export.restype, R.ogm_restate_export.argtypes = u64, [vp] * 10
    R.ogm_restate_point_keys.restype, R.ogm_restate_point_keys.argtypes = None, [vp, vp, u64, vp, vp]
    R.ogm_restate_walk.restype, R.ogm_restate_walk.argtypes = u64, [vp, vp, f, vp, u64]
    R.ogm_reference_walk_steps.restype, R.ogm_reference_walk_steps.argtypes = u64, [vp, vp, f, u64]
    return R


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return build_restatement(tmp_path_factory.mktemp("ogm"))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a, cols=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.float32)
    return a if cols is None else a.reshape(-1, cols)


def T16(pose):
    return np.ascontiguousarray(np.asarray(np.eye(4) if pose is None else pose, np.float32).reshape(4, 4).T).reshape(-1)


class RestatedMap:
    """the restatement behind the interface of api.OccupancyGridMap (numpy in, numpy out)"""

    def __init__(self, R, voxel_size):
        self.R = R
        self.h = R.ogm_restate_create(voxel_size)
        if not self.h:
            raise ValueError("voxel_size must be positive.")

    def __del__(self):
        if getattr(self, "h", None):
            self.R.ogm_restate_destroy(self.h)
            self.h = None

    def set(self, name, value):
        if self.R.ogm_restate_set(self.h, PARAM[name], float(value)):
            raise ValueError(name)

    def set_log_odds_limits(self, lo, hi):
        if self.R.ogm_restate_set_limits(self.h, lo, hi):
            raise ValueError("minimum must not exceed maximum.")

    def info(self, name):
        return int(self.R.ogm_restate_info(self.h, INFO[name]))

    def threshold_log_odds(self):
        return float(self.R.ogm_restate_threshold_log_odds(self.h))

    def clear(self):
        self.R.ogm_restate_clear(self.h)

    def add_point_cloud(self, pts, pose=None, covs=None, rgb=None, intensities=None):
        pts, covs, rgb, inten = _f32(pts, 4), _f32(covs, 16), _f32(rgb, 4), _f32(intensities)
        self.R.ogm_restate_add(self.h, _p(pts), _p(covs), _p(rgb), _p(inten), len(pts), _p(T16(pose)))

    def extract_occupied_points(self, pose=None, max_distance=100.0):
        n = max(self.info("voxel_num"), 1)
        pts, cov, rgb = np.zeros((n, 4), np.float32), np.zeros((n, 16), np.float32), np.zeros((n, 4), np.float32)
        inten, keys = np.zeros(n, np.float32), np.zeros(n, np.uint64)
        c = np.ascontiguousarray(np.asarray(np.eye(4) if pose is None else pose, np.float32).reshape(4, 4)[:3, 3])
        k = self.R.ogm_restate_extract(self.h, _p(c), max_distance, _p(pts), _p(cov), _p(rgb), _p(inten), _p(keys))
        return {"points": pts[:k], "covs": cov[:k] if self.info("has_cov") else None, "rgb": rgb[:k] if self.info("has_rgb") else None,
                "intensities": inten[:k] if self.info("has_intensity") else None, "keys": keys[:k]}

    def compute_overlap_ratio(self, pts, pose=None):
        pts = _f32(pts, 4)
        return float(self.R.ogm_restate_overlap(self.h, _p(pts), len(pts), _p(T16(pose))))

    def voxel_probability(self, xyz):
        return float(self.R.ogm_restate_probability(self.h, _p(np.asarray(xyz, np.float32).copy())))

    def point_keys(self, pts, pose=None):
        pts = _f32(pts, 4)
        keys = np.zeros(len(pts), np.uint64)
        self.R.ogm_restate_point_keys(self.h, _p(pts), len(pts), _p(T16(pose)), _p(keys))
        return keys

    def export(self):
        n = max(self.info("voxel_num"), 1)
        arrays = {name: np.zeros((n,) + shape, dt) for name, dt, shape in EXPORT_FIELDS}
        k = self.R.ogm_restate_export(self.h, *[_p(arrays[name]) for name, _, _ in EXPORT_FIELDS])
        return {name: a[:k] for name, a in arrays.items()}


def P(rows):
    a = np.ones((len(rows), 4), np.float32)
    a[:, :3] = np.asarray(rows, np.float32).reshape(-1, 3)
    return a


def cov16(xx, xy, xz, yy, yz, zz):
    m = np.zeros((4, 4), np.float32)
    m[:3, :3] = [[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]
    return m.T.reshape(-1)


def spd_fn(mat, fn):
    w, V = np.linalg.eigh(np.asarray(mat, np.float64))
    return (V * fn(w)) @ V.T


def log_euclidean_mean(mats, R=None):
    """exp(mean(log C)) in float64; with R, of R C R^T"""
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    return spd_fn(sum(spd_fn(R @ np.asarray(m, np.float64) @ R.T, lambda w: np.log(np.maximum(w, 1e-6))) for m in mats) / len(mats),
                  np.exp)


def rot_z(th):
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]
    return pose


def known_answers(make, add, extract, overlap):
    """cpp/tests/test_occupancy_grid_map.cpp:90-523 against any implementation: make(voxel_size) -> map with the setters of
    RestatedMap / a thin adapter; add(map, pts, pose, covs, rgb, intensities); extract(map, pose, max_distance) -> dict of numpy
    arrays; overlap(map, pts, pose) -> float. Invalid arguments must raise."""
    for bad in (0.0, -0.1):  # :90-95
        with pytest.raises(Exception):
            make(bad)
    # :97-135 two voxels
    m = make(0.2)
    add(m, P([[0.05, 0.05, 0.0], [0.07, 0.05, 0.0], [0.35, 0.05, 0.0]]))
    out = extract(m, None, 1.0)["points"]
    out = out[np.lexsort((out[:, 2], out[:, 1], out[:, 0]))]
    assert out.shape == (2, 4) and np.abs(out[:, :3] - [[0.06, 0.05, 0], [0.35, 0.05, 0]]).max() <= 1e-5 and (out[:, 3] == 1).all()
    # :141-165 far voxels skipped
    m = make(0.2)
    add(m, P([[0, 0, 0], [5.0, 0, 0]]))
    out = extract(m, None, 1.0)["points"]
    assert out.shape == (1, 4) and abs(out[0, 0]) <= 1e-5
    # :167-202 overlap ratio
    m = make(0.5)
    mp = P([[0.1, 0.1, 0.0], [1.1, 0.0, 0.0]])
    add(m, mp)
    q = P([[-0.9, 0.1, 0.0], [0.1, 0.0, 0.0], [1.0, 0.0, 0.0]])
    sensor = np.eye(4, dtype=np.float32)
    sensor[0, 3] = 1.0
    assert abs(overlap(m, q, sensor) - 2.0 / 3.0) <= 1e-5
    m.set("occupancy_threshold", 0.8)
    assert abs(overlap(m, q, sensor)) <= 1e-5
    add(m, mp)
    assert abs(overlap(m, q, sensor) - 2.0 / 3.0) <= 1e-5
    # :208-247 colour and intensity
    rgb = [[0.0, 0.2, 0.4, 1.0], [0.2, 0.4, 0.6, 1.0]]
    m = make(0.1)
    add(m, P([[0, 0, 0], [0.05, 0, 0]]), None, None, rgb, [10.0, 30.0])
    r = extract(m, None, 1.0)
    assert len(r["points"]) == 1 and r["covs"] is None
    assert np.abs(r["points"][0, :3] - [0.025, 0, 0]).max() <= 1e-5
    assert np.abs(r["rgb"][0] - [0.1, 0.3, 0.5, 1.0]).max() <= 1e-5 and abs(r["intensities"][0] - 20.0) <= 1e-5
    # :253-301 covariance mean (log-Euclidean)
    c = [(1.0, 0.2, 0.3, 2.0, 0.4, 3.0), (3.0, 0.6, 0.9, 4.0, 0.8, 5.0)]
    mats = [np.array([[a, b, cc], [b, d, e], [cc, e, f]]) for a, b, cc, d, e, f in c]
    m = make(0.1)
    add(m, P([[0, 0, 0], [0.05, 0, 0]]), None, np.stack([cov16(*x) for x in c]), rgb, [10.0, 30.0])
    r = extract(m, None, 1.0)
    assert len(r["points"]) == 1 and r["rgb"] is not None and r["intensities"] is not None
    got = r["covs"][0].reshape(4, 4).T
    assert np.abs(got[:3, :3] - log_euclidean_mean(mats)).max() <= 1e-5
    assert np.linalg.norm(got[3]) <= 1e-5 and np.linalg.norm(got[:, 3]) <= 1e-5
    # :303-347 rotated into the map frame
    pose = rot_z(np.float32(np.pi) / np.float32(2.0))
    pose[:3, 3] = [1.0, 0.0, 0.0]
    c = [(1.0, 0.0, 0.0, 4.0, 0.0, 9.0), (9.0, 0.0, 0.0, 16.0, 0.0, 25.0)]
    mats = [np.diag([a, d, f]) for a, _, _, d, _, f in c]
    m = make(0.5)
    add(m, P([[0, 0, 0], [0.1, 0, 0]]), pose, np.stack([cov16(*x) for x in c]))
    r = extract(m, pose, 1.0)
    Rm = pose[:3, :3].astype(np.float64)
    assert len(r["points"]) == 1
    assert np.abs(r["covs"][0].reshape(4, 4).T[:3, :3] - Rm @ log_euclidean_mean(mats) @ Rm.T).max() <= 1e-4
    # :349-366 no covariance output without covariance input
    m = make(0.1)
    add(m, P([[0, 0, 0], [0.05, 0, 0]]))
    r = extract(m, None, 1.0)
    assert len(r["points"]) == 1 and r["covs"] is None
    # :368-392 carving along a ray; :394-412 carving disabled
    for carving in (True, False):
        m = make(0.1)
        m.set("log_odds_hit", 0.9)
        m.set("log_odds_miss", -0.6)
        if not carving:
            m.set("free_space_updates_enabled", 0)
        add(m, P([[0.45, 0, 0]]))
        free = m.voxel_probability([0.05, 0, 0])
        assert (free < 0.5) if carving else (abs(free - 0.5) <= 1e-5)
        assert m.voxel_probability([0.45, 0, 0]) > 0.5
        if carving:  # the values behind the inequalities: one miss per free cell, one hit
            for x in (0.05, 0.15, 0.25, 0.35):
                assert abs(m.voxel_probability([x, 0, 0]) - 1.0 / (1.0 + np.exp(0.6))) <= 1e-5
            assert abs(m.voxel_probability([0.45, 0, 0]) - 1.0 / (1.0 + np.exp(-0.9))) <= 1e-5
    # :421-456 repeated observations raise confidence
    m = make(0.1)
    m.set("log_odds_hit", 1.0)
    m.set("log_odds_miss", -0.5)
    add(m, P([[0, 0, 0], [0.2, 0, 0]]))
    add(m, P([[0, 0, 0]]))
    out = extract(m, None, 1.0)["points"]
    out = out[np.argsort(out[:, 0])]
    assert len(out) == 2 and m.voxel_probability(out[1, :3]) < m.voxel_probability(out[0, :3])
    # :458-489 pruning disabled keeps every voxel
    m = make(0.1)
    m.set("log_odds_hit", 1.0)
    m.set("log_odds_miss", -0.5)
    add(m, P([[0, 0, 0], [0.2, 0, 0]]))
    base = m.voxel_probability([0.2, 0, 0])
    m.set("voxel_pruning_enabled", 0)
    add(m, P([[0, 0, 0]]))
    assert abs(m.voxel_probability([0.2, 0, 0]) - base) <= 1e-5
    # :491-528 pruning by frame age
    m = make(0.1)
    m.set("log_odds_hit", 1.0)
    m.set("log_odds_miss", -0.5)
    m.set("free_space_updates_enabled", 0)
    m.set("voxel_pruning_enabled", 1)
    m.set("stale_frame_threshold", 100)
    add(m, P([[0, 0, 0]]))
    for _ in range(101):
        add(m, P([[1.0, 0, 0]]))
    assert abs(m.voxel_probability([0, 0, 0]) - 0.5) <= 1e-5 and m.voxel_probability([1.0, 0, 0]) > 0.5
    assert m.info("voxel_num") == 1 and m.info("frame_index") == 102
    # the setters' validation (:107-121)
    m = make(0.1)
    for name, v in (("occupancy_threshold", 0.0), ("occupancy_threshold", 1.0), ("voxel_size", 0.0)):
        with pytest.raises(Exception):
            m.set(name, v)
    with pytest.raises(Exception):
        m.set_log_odds_limits(1.0, -1.0)
    m.set_log_odds_limits(-2.0, 3.5)


def test_reference_known_answers(R):
    known_answers(lambda vs: RestatedMap(R, vs), lambda m, pts, pose=None, covs=None, rgb=None, inten=None:
                  m.add_point_cloud(pts, pose, covs, rgb, inten), lambda m, pose, d: m.extract_occupied_points(pose, d),
                  lambda m, q, pose: m.compute_overlap_ratio(q, pose))


def test_early_returns(R):
    """:130-132, 176-178, 418-420"""
    m = RestatedMap(R, 0.5)
    m.add_point_cloud(np.zeros((0, 4), np.float32))
    assert m.info("frame_index") == 0 and m.info("voxel_num") == 0
    assert len(m.extract_occupied_points()["points"]) == 0 and m.compute_overlap_ratio(P([[0, 0, 0]])) == 0.0
    m.add_point_cloud(P([[0.1, 0.1, 0.1]]))
    assert m.info("frame_index") == 1 and m.compute_overlap_ratio(np.zeros((0, 4), np.float32)) == 0.0


# ------------------------------------------------------------------------------------------------------------------ the walk
WALK_SEED, WALK_RAYS, WALK_VOXEL, EDGE_MARGIN = 20240, 2000, 0.5, 1e-4


def walk_cells(R, origin, target, inv_voxel, cap=4096):
    cells = np.zeros((cap, 3), np.int32)
    o, t = np.asarray(origin, np.float32).copy(), np.asarray(target, np.float32).copy()
    steps = int(R.ogm_restate_walk(_p(o), _p(t), inv_voxel, _p(cells), cap))
    assert steps <= cap
    return steps, cells[:steps]


def crossed_cells_f64(o, t):
    """The cells whose interior the segment o -> t (cell units, float64) crosses, in order, the origin's cell excluded; and the
    smallest distance (cell units) between a crossing of a cell face and an edge of that face."""
    d = t - o
    events = []
    for a in range(3):
        lo, hi = np.floor(o[a]), np.floor(t[a])
        planes = np.arange(lo + 1, hi + 1) if hi > lo else np.arange(lo, hi, -1)
        events += [((k - o[a]) / d[a], a) for k in planes]
    events.sort()
    cell = np.floor(o).astype(np.int64)
    cells, margin = [], np.inf
    for s, a in events:
        p = o + s * d
        for b in range(3):
            if b != a:
                margin = min(margin, abs(p[b] - np.round(p[b])))
        cell = cell.copy()
        cell[a] += 1 if d[a] > 0 else -1
        cells.append(cell)
    return np.array(cells, np.int64).reshape(-1, 3), margin


def test_bounded_walk_visits_the_cells_the_segment_crosses(R):
    rs = np.random.RandomState(WALK_SEED)
    inv = np.float32(1.0 / WALK_VOXEL)
    excluded = 0
    for _ in range(WALK_RAYS):
        o = (rs.uniform(-2, 2, 3) + rs.uniform(0.05, 0.45)).astype(np.float32)  # off the lattice of 0.5 m
        t = rs.uniform(-10, 10, 3).astype(np.float32)
        so, st = o.astype(np.float64) * float(inv), t.astype(np.float64) * float(inv)  # exact: inv is 2
        want, margin = crossed_cells_f64(so, st)
        manhattan = int(np.abs(np.floor(st) - np.floor(so)).sum())
        steps, got = walk_cells(R, o, t, inv)
        assert steps == manhattan == len(want)  # whatever the margin: the count is the bound
        if steps:
            assert np.array_equal(got[-1], np.floor(st).astype(np.int64))  # and it lands on the target's cell
        if margin < EDGE_MARGIN:
            excluded += 1
            continue
        assert np.array_equal(got.astype(np.int64), want), (o, t)
    share = excluded / WALK_RAYS
    print(f"bounded walk: {excluded} of {WALK_RAYS} rays pass within {EDGE_MARGIN} cell of a cell edge ({100 * share:.2f} %), excluded")
    assert share <= 0.05


def test_ray_that_ends_one_ulp_from_a_cell_face(R):
    """Targets one ulp inside a cell face (and one exactly on it), reached along a diagonal: where an axis' accumulated float32
    t_max ties with or undercuts another's after that axis has arrived, the reference's loop (:880-899) steps the arrived axis once
    more, leaves the target's column and cannot land any more. The bounded walk ends in its Manhattan count of steps on the target's
    cell, on every one of them; what the reference's loop does within ten times that budget is printed."""
    inv = np.float32(1.0)
    o = np.array([0.3, 0.7, 0.5], np.float32)
    below = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))  # noqa: E731
    targets = [(below(7.0), 6.25, 0.5), (below(7.0), below(7.0), 0.5), (below(-3.0), 9.75, below(4.0)), (7.0, below(7.0), below(1.0)),
               (below(40.0), below(40.0), below(40.0))]
    for t in targets:
        t = np.array(t, np.float32)
        assert np.any(np.ceil(t) - t <= np.spacing(t))  # within one ulp of a face
        manhattan = int(np.abs(np.floor(t.astype(np.float64)) - np.floor(o.astype(np.float64))).sum())
        steps, cells = walk_cells(R, o, t, inv)
        assert steps == manhattan and np.array_equal(cells[-1], np.floor(t).astype(np.int32))
        assert np.abs(np.diff(np.vstack([np.floor(o).astype(np.int32)[None], cells]), axis=0)).sum(axis=1).tolist() == [1] * steps
        ref = int(R.ogm_reference_walk_steps(_p(o), _p(t), inv, 10 * manhattan))
        print(f"target {t}: bounded walk {steps} steps = Manhattan count; the reference's loop: "
              f"{'not landed after ' + str(ref) if ref == 10 * manhattan else 'landed after ' + str(ref)} steps")


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_cabi_argument_checks_without_gpu():
    from sycl_points_amd import _lib

    _lib.build()
    L = _lib.lib()
    h = C.c_void_p()
    for bad in (0.0, -0.1, float("nan")):
        assert L.sp_ogm_create(bad, None, C.byref(h)) == _lib.SP_ERR_INVALID_ARGUMENT and not h.value
    assert b"voxel_size must be positive" in L.sp_last_error()
    assert L.sp_ogm_create(0.5, None, None) == _lib.SP_ERR_INVALID_ARGUMENT
    r, n = C.c_float(7.0), C.c_size_t(7)
    assert L.sp_ogm_set(None, 0, 1.0) == L.sp_ogm_clear(None, None) == L.sp_ogm_set_log_odds_limits(None, 0.0, 1.0) == 1
    assert L.sp_ogm_add_point_cloud(None, None, None, None, None, 0, None, None) == 1
    assert L.sp_ogm_overlap_ratio(None, None, 0, None, C.byref(r), None) == 1
    assert L.sp_ogm_voxel_probability(None, None, C.byref(r), None) == 1
    assert L.sp_ogm_extract_occupied_points(None, None, 1.0, None, None, None, None, None, 0, C.byref(n), None) == 1
    assert L.sp_ogm_export(None, None, None, None, None, None, None, None, None, None, 0, C.byref(n), None) == 1
    assert L.sp_ogm_get(None, 0) == 0.0 and L.sp_ogm_info(None, 0) == 0
    L.sp_ogm_destroy(None)


def test_walk_kernel_uses_no_scratch():
    from sycl_points_amd import _lib

    _lib.build()
    report = os.path.join(ROOT, "sycl_points_amd", "lib", "occupancy_grid_map.resources.txt")
    rows = [l for l in open(report) if "ogm_" in l]
    assert any("ogm_walk_kernel" in l for l in rows) and any("ogm_hit_kernel" in l for l in rows)
    for row in rows:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", row).group(1)) == 0, row
        assert int(re.search(r"VGPRs Spill: (\d+)", row).group(1)) == 0, row
