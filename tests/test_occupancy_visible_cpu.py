"""OccupancyGridMap::extract_visible_points without a device: the CPU restatement (tests/cpp/occupancy_visible_restate.cpp; the
specification of DESIGN.md 4.10 and 7 over mapping/occupancy_grid_map.hpp:183-411 of the reference) on states built with the
restated map of tests/test_occupancy_grid_cpu.py, whose helpers are used here.

What pins it: the reference's own three known answers (cpp/tests/test_occupancy_grid_map.cpp:530-627, its tolerance 1e-5), a wall
whose counts follow from its geometry, the counts of the GPU suite's random cloud (from the float32 numpy transcription below, run on
the restated map's state), that transcription itself, which shares no code with the restatement but the walked cells
(ogm_restate_walk), and properties that need no tolerance. Then the C ABI's argument checks (SP_ERR_INVALID_ARGUMENT before any HIP
call) and the compiler's resource report for the file's kernels.
The GPU suite (tests/test_gpu_occupancy_visible.py) holds the device to this restatement; its helpers live here."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = np.float32(3.1415927)
VOXEL = 0.5
SPHERE = (100.0, float(PI), float(2 * PI))  # max_distance, horizontal_fov, vertical_fov: every occupied voxel is a candidate
ARGS = {"sphere": SPHERE, "frustum": (6.0, float(PI / 2), float(PI / 2)), "narrow": (10.0, float(PI / 3), float(PI / 6))}
WALL_SENSOR = (0.137, -0.211, 0.123)


def load_helpers(file_name, module_name):
    spec = importlib.util.spec_from_file_location(module_name, os.path.join(ROOT, "tests", file_name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_visible_restatement(out_dir):
    so = os.path.join(str(out_dir), "libogm_visible_restate.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "occupancy_visible_restate.cpp"), "-o", so])
    V = C.CDLL(so)
    vp, u64, f = C.c_void_p, C.c_uint64, C.c_float
    V.ogm_visible_restate.restype = u64
    V.ogm_visible_restate.argtypes = [vp, vp, vp, vp, u64, f, f, vp, f, f, f, vp, vp]
    return V


@pytest.fixture(scope="module")
def cpu():
    return load_helpers("test_occupancy_grid_cpu.py", "ogm_cpu_helpers")


@pytest.fixture(scope="module")
def R(cpu, tmp_path_factory):
    return cpu.build_restatement(tmp_path_factory.mktemp("ogm_visible_state"))


@pytest.fixture(scope="module")
def V(tmp_path_factory):
    return build_visible_restatement(tmp_path_factory.mktemp("ogm_visible"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def T16(pose):
    return np.ascontiguousarray(np.asarray(np.eye(4) if pose is None else pose, np.float32).reshape(4, 4).T).reshape(-1)


def restated_visible(V, export, voxel_size, threshold, pose, max_distance, horizontal_fov, vertical_fov):
    """the restatement on an export (of the restated map or of the device): the visible keys in the export's row order, and
    (candidates, occluded, longest walk)"""
    n = len(export["keys"])
    keys = np.ascontiguousarray(export["keys"], np.uint64)
    hits = np.ascontiguousarray(export["hit_count"], np.uint32)
    lo = np.ascontiguousarray(export["log_odds"], np.float32)
    xyz = np.ascontiguousarray(export["sum_xyz"], np.float32)
    out, counts = np.zeros(max(n, 1), np.uint64), np.zeros(3, np.uint64)
    k = V.ogm_visible_restate(_p(keys), _p(hits), _p(lo), _p(xyz), n, voxel_size, threshold, _p(T16(pose)), max_distance,
                              horizontal_fov, vertical_fov, _p(out), _p(counts))
    return out[:k], tuple(int(c) for c in counts)


def fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64"""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def numpy_visible(R, cpu, export, voxel_size, threshold, pose, max_distance, horizontal_fov, vertical_fov):
    """Items 4-5 of the specification transcribed in float32 numpy; the walked cells are ogm_restate_walk's. Returns the visible
    keys (row order), the candidate keys and the longest walk."""
    f32 = np.float32
    T = np.asarray(np.eye(4) if pose is None else pose, f32).reshape(4, 4)
    sensor, voxel = T[:3, 3].copy(), f32(voxel_size)
    inv = f32(1.0) / voxel
    cell = np.floor(sensor * inv)
    if not (np.isfinite(cell).all() and (cell >= -(1 << 20)).all() and (cell < (1 << 20)).all()):
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64), 0
    hf = min(max(f32(horizontal_fov), f32(1e-6)), PI - f32(1e-6))
    vf = min(max(f32(vertical_fov), f32(1e-6)), f32(2) * PI - f32(1e-6))
    cos_h_limit, cos_v_limit = f32(np.cos(np.float64(hf * f32(0.5)))), f32(np.cos(np.float64(vf * f32(0.5))))
    backward = hf >= PI - f32(1e-6)
    keys, hits = export["keys"], export["hit_count"]
    with np.errstate(divide="ignore", invalid="ignore"):
        cen = export["sum_xyz"].astype(f32) * (f32(1.0) / hits.astype(f32))[:, None]
        occupied = (hits > 0) & ~(export["log_odds"] < f32(threshold))
        d = cen - sensor
        dist_sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        zero = np.zeros(len(keys), f32)
        local = [fma32(d[:, 2], T[2, i], fma32(d[:, 1], T[1, i], fma32(d[:, 0], T[0, i], zero))) for i in range(3)]  # R^T d
        forward = np.abs(local[0]) if backward else local[0]
        cand = occupied & (dist_sq <= f32(max_distance) * f32(max_distance))
        if not backward:
            cand &= ~(local[0] <= 0)
        for side, limit in ((local[1], cos_h_limit), (local[2], cos_v_limit)):
            norm_sq = forward * forward + side * side
            cosine = np.where(norm_sq > 0, np.clip(forward / np.sqrt(norm_sq), f32(-1), f32(1)), f32(1))
            cand &= ~(cosine < limit)
        dist = np.sqrt(dist_sq)
    by_key = {int(k): i for i, k in enumerate(keys)}
    visible, longest = [], 0
    for i in np.flatnonzero(cand):
        hidden = False
        if dist[i] > voxel:
            steps, cells = cpu.walk_cells(R, sensor, cen[i], inv)
            longest = max(longest, steps)
            for x, y, z in cells[:-1].astype(np.int64) + (1 << 20):
                j = by_key.get(int(x | (y << 21) | (z << 42)))
                if j is None or j == i or not occupied[j]:
                    continue
                if dist_sq[j] + f32(1e-6) < dist_sq[i]:
                    hidden = True
                    break
        if not hidden:
            visible.append(keys[i])
    return np.array(visible, np.uint64), keys[cand], longest


def P(rows):
    a = np.ones((len(rows), 4), np.float32)
    a[:, :3] = np.asarray(rows, np.float32).reshape(-1, 3)
    return a


def identity_at(xyz):
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = xyz
    return T


def centroids(export, keys):
    row = {int(k): i for i, k in enumerate(export["keys"])}
    i = [row[int(k)] for k in keys]
    return export["sum_xyz"][i] / export["hit_count"][i][:, None].astype(np.float32)


def wall_points(voxel=VOXEL):
    """the centres of a 21 x 21 plane of cells at x-cell 4 and of an 11 x 11 plane at x-cell 8, y and z cells centred on 0"""
    planes = []
    for x_cell, half in ((4, 10), (8, 5)):
        j, k = np.meshgrid(np.arange(-half, half + 1), np.arange(-half, half + 1), indexing="ij")
        planes.append(np.stack([np.full(j.size, x_cell), j.ravel(), k.ravel()], axis=1))
    return P((np.concatenate(planes) + 0.5) * voxel)


def known_answers(make, add, visible):
    """cpp/tests/test_occupancy_grid_map.cpp:530-627 and the wall against any implementation: make(voxel_size) -> a map with the
    setters of RestatedMap; add(map, pts); visible(map, pose, max_distance, horizontal_fov, vertical_fov) -> (points (n, >= 3),
    number of occupied voxels)"""
    pi = np.float32(3.14159265358979323846)
    m = make(0.1)  # :530-561 the frustum
    add(m, P([[1, 0, 0], [0.5, 0.5, 0], [-1, 0, 0]]))
    out, _ = visible(m, None, 5.0, float(pi / np.float32(6)), float(pi / np.float32(6)))
    assert len(out) == 1 and np.abs(out[0, :3] - [1, 0, 0]).max() <= 1e-5
    m = make(0.1)  # :563-595 backward when the horizontal field is pi
    add(m, P([[1, 0, 0], [-1, 0, 0]]))
    out, _ = visible(m, None, 5.0, float(pi), float(pi))
    assert len(out) == 2 and np.abs(np.sort(out[:, 0]) - [-1, 1]).max() <= 1e-5
    m = make(0.2)  # :597-627 occlusion
    add(m, P([[0.8, 0, 0], [1.6, 0, 0]]))
    out, _ = visible(m, None, 5.0, float(pi / np.float32(2)), float(pi / np.float32(2)))
    assert len(out) == 1 and np.abs(out[0, :3] - [0.8, 0, 0]).max() <= 1e-5
    # the wall, seen from beside the origin: the front plane hides the whole back plane
    for carving, occupied, seen in ((False, 562, 72), (True, 467, 139)):
        m = make(VOXEL)
        m.set("free_space_updates_enabled", int(carving))
        add(m, wall_points())
        out, n_occupied = visible(m, identity_at(WALL_SENSOR), 100.0, float(pi / np.float32(2)), float(pi / np.float32(2)))
        assert (n_occupied, len(out)) == (occupied, seen)
        if carving:  # the frame's own rays carved holes into the front plane: both planes show
            assert set(np.unique(out[:, 0]).tolist()) == {2.25, 4.25}
        else:
            assert (out[:, 0] == 2.25).all()


def pose_of(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T.astype(np.float32)


POSE = pose_of(0.3, -0.2, 0.7, (0.137, -0.211, 0.373))  # the POSE of tests/test_gpu_occupancy_grid.py


def random_cloud(n):
    """the first n points of the GPU suite's cloud (tests/test_gpu_occupancy_grid.py, make_cloud(4096, seed=31))"""
    pts = np.ones((4096, 4), np.float32)
    pts[:, :3] = np.random.RandomState(31).uniform(-8.0, 8.0, (4096, 3)).astype(np.float32)
    return pts[:n]


@pytest.fixture(scope="module")
def states(cpu, R):
    """export() of the restated map after the random cloud's first n points from POSE, by (n, carving); built once, never changed"""
    out = {}
    for n, carving in ((63, False), (64, False), (65, False), (4096, False), (4096, True)):
        m = cpu.RestatedMap(R, VOXEL)
        m.set("free_space_updates_enabled", int(carving))
        m.add_point_cloud(random_cloud(n), POSE)
        out[n, carving] = (m, m.export())
    return out


def test_reference_known_answers_and_the_wall(cpu, R, V):
    def visible(m, pose, d, hf, vf):
        e = m.export()
        keys, (cand, occluded, _) = restated_visible(V, e, m.voxel_size, m.threshold_log_odds(), pose, d, hf, vf)
        assert len(keys) == cand - occluded
        return centroids(e, keys), int(((e["hit_count"] > 0) & ~(e["log_odds"] < m.threshold_log_odds())).sum())

    def make(voxel_size):
        m = cpu.RestatedMap(R, voxel_size)
        m.voxel_size = voxel_size
        return m

    known_answers(make, lambda m, pts: m.add_point_cloud(pts), visible)


def test_wall_counts(cpu, R, V):
    """562 occupied voxels; the frustum of pi/2 x pi/2 holds 193 of them, the 121 of the back plane among them, every one hidden"""
    m = cpu.RestatedMap(R, VOXEL)
    m.set("free_space_updates_enabled", 0)
    m.add_point_cloud(wall_points())
    e = m.export()
    pose = identity_at(WALL_SENSOR)
    keys, (cand, occluded, _) = restated_visible(V, e, VOXEL, 0.0, pose, 100.0, float(PI / 2), float(PI / 2))
    assert len(e["keys"]) == 562 and (cand, occluded, len(keys)) == (193, 121, 72)
    _, cand_keys, _ = numpy_visible(R, cpu, e, VOXEL, 0.0, pose, 100.0, float(PI / 2), float(PI / 2))
    x = centroids(e, cand_keys)[:, 0]
    assert (x == 4.25).sum() == 121 and (x == 2.25).sum() == 72 and (centroids(e, keys)[:, 0] == 2.25).all()


@pytest.mark.parametrize("n", (63, 64, 65))
def test_random_cloud_small(V, states, n):
    _, e = states[n, False]
    keys, (cand, occluded, _) = restated_visible(V, e, VOXEL, 0.0, POSE, *SPHERE)
    assert cand == len(e["keys"]) and occluded == 1 and len(keys) == cand - 1


@pytest.mark.parametrize("case, carving, args, want", [
    ("sphere", False, SPHERE, (3859, 336)), ("frustum", False, ARGS["frustum"], (138, 39)), ("sphere", True, SPHERE, (2917, 1636))])
def test_random_cloud_counts(V, states, case, carving, args, want):
    _, e = states[4096, carving]
    keys, (cand, occluded, longest) = restated_visible(V, e, VOXEL, 0.0, POSE, *args)
    assert (cand, len(keys)) == want and cand - occluded == len(keys)
    if case == "sphere" and not carving:
        assert longest == 42


@pytest.mark.parametrize("n, carving, args", [(63, False, SPHERE), (64, False, SPHERE), (65, False, SPHERE), (4096, False, SPHERE),
                                              (4096, False, ARGS["frustum"]), (4096, True, SPHERE)])
def test_numpy_transcription_agrees(cpu, R, V, states, n, carving, args):
    _, e = states[n, carving]
    keys, (cand, _, longest) = restated_visible(V, e, VOXEL, 0.0, POSE, *args)
    want, cand_keys, want_longest = numpy_visible(R, cpu, e, VOXEL, 0.0, POSE, *args)
    assert np.array_equal(keys, want) and cand == len(cand_keys) and longest == want_longest


def test_visible_is_a_subset_of_occupied(V, states):
    """L2 <= d implies L-infinity <= d"""
    for (n, carving), (m, e) in states.items():
        for d, hf, vf in ARGS.values():
            keys, _ = restated_visible(V, e, VOXEL, 0.0, POSE, d, hf, vf)
            assert len(np.unique(keys)) == len(keys)
            assert np.isin(keys, m.extract_occupied_points(POSE, d)["keys"]).all()


def test_one_voxel_is_visible_whenever_it_is_a_candidate(cpu, R, V):
    m = cpu.RestatedMap(R, VOXEL)
    m.add_point_cloud(P([[3.3, 0.4, -0.2]]))  # carving on: the free cells of its ray are voxels too, none occupied
    e = m.export()
    assert len(e["keys"]) > 1 and (e["hit_count"] > 0).sum() == 1
    seen = 0
    for yaw in np.linspace(0, 2 * np.pi, 13):
        keys, (cand, occluded, _) = restated_visible(V, e, VOXEL, 0.0, pose_of(0, 0, yaw, (0.1, 0.1, 0.1)), 10.0, 1.0, 1.0)
        assert occluded == 0 and len(keys) == cand <= 1
        seen += cand
    assert 0 < seen < 13
    assert restated_visible(V, e, VOXEL, 0.0, None, 3.0, 1.0, 1.0)[1][0] == 0  # beyond max_distance


def test_a_candidate_within_voxel_size_is_visible_behind_an_occluder(cpu, R, V):
    """voxel 1.0; a target in cell (0, 0, 0), an occupied voxel in cell (0, -1, 0), the sensor in cell (-1, -1, 0) on the diagonal
    through both: the walk to the target steps x first (a tie) into the occupied cell, whose centroid is nearer. From 1.77 away
    the target is hidden; from 0.49 away, within voxel_size, it is not walked to and is visible."""
    target, occluder = [0.3, 0.3, 0.5], [0.05, -0.05, 0.5]
    m = cpu.RestatedMap(R, 1.0)
    m.set("free_space_updates_enabled", 0)
    m.add_point_cloud(P([target, occluder]))
    e = m.export()
    for sensor, hidden in (((-0.95, -0.95, 0.5), 1), ((-0.05, -0.05, 0.5), 0)):
        steps, cells = cpu.walk_cells(R, np.float32(sensor), np.float32(target), np.float32(1.0))
        assert steps == 2 and cells.tolist() == [[0, -1, 0], [0, 0, 0]]
        assert np.linalg.norm(np.float32(occluder) - np.float32(sensor)) + 0.3 < np.linalg.norm(np.float32(target) - np.float32(sensor))
        keys, (cand, occluded, _) = restated_visible(V, e, 1.0, 0.0, identity_at(sensor), 100.0, *SPHERE[1:])
        assert (cand, occluded) == (2, hidden)
        seen = centroids(e, keys)
        assert np.abs(seen - occluder).max(axis=1).min() < 1e-6 and len(seen) == 2 - hidden


def test_fov_beyond_the_clamps_gives_the_clamped_result(V, states):
    _, e = states[4096, False]
    tol = 1e-6
    for (hf, vf), (ch, cv) in ((((10.0, 10.0)), (float(PI) - tol, float(2 * PI) - tol)), ((-1.0, 0.0), (tol, tol)),
                               ((float(PI), 1.0), (float(PI) - tol, 1.0))):
        got, counts = restated_visible(V, e, VOXEL, 0.0, POSE, 100.0, hf, vf)
        want, want_counts = restated_visible(V, e, VOXEL, 0.0, POSE, 100.0, ch, cv)
        assert np.array_equal(got, want) and counts == want_counts
    assert restated_visible(V, e, VOXEL, 0.0, POSE, 100.0, 10.0, 10.0)[1][0] == 3859  # the whole sphere


def test_sensor_outside_the_cell_range_sees_nothing(V, states):
    _, e = states[64, False]
    for xyz in ((1e7, 0, 0), (0, -1e7, 0), (np.nan, 0, 0), (0, 0, np.inf)):
        keys, counts = restated_visible(V, e, VOXEL, 0.0, identity_at(xyz), *SPHERE)
        assert len(keys) == 0 and counts == (0, 0, 0)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_cabi_symbol_and_argument_checks_without_gpu():
    from sycl_points_amd import _lib

    _lib.build()
    L = _lib.lib()
    assert hasattr(L, "sp_ogm_extract_visible_points")
    header = open(os.path.join(ROOT, "include", "sycl_points_amd.h")).read()
    assert "int sp_ogm_extract_visible_points(sp_occupancy_grid_map* map, const float* sensor_pose_host16" in header
    assert L.sp_abi_version() == 7
    pose, n = T16(None), C.c_size_t(7)
    not_a_map = np.zeros(4096, np.uint8)  # never read: the NULL checks come first
    call = lambda m, p, n_out: L.sp_ogm_extract_visible_points(m, p, 1.0, 1.0, 1.0, None, None, None, None, None, 0, n_out, None)  # noqa: E731
    assert call(None, _p(pose), C.byref(n)) == _lib.SP_ERR_INVALID_ARGUMENT
    assert call(_p(not_a_map), None, C.byref(n)) == _lib.SP_ERR_INVALID_ARGUMENT
    assert call(_p(not_a_map), _p(pose), None) == _lib.SP_ERR_INVALID_ARGUMENT
    assert n.value == 7


def test_kernels_use_no_scratch():
    from sycl_points_amd import _lib

    _lib.build()
    report = os.path.join(ROOT, "sycl_points_amd", "lib", "occupancy_grid_map.resources.txt")
    rows = [l for l in open(report) if "Function Name" in l]
    for name in ("ogm_walk_kernel", "ogm_visible_flag_kernel", "ogm_candidate_list_kernel", "ogm_visible_walk_kernel"):
        assert any(name in l for l in rows), name
    for row in rows:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", row).group(1)) == 0, row
        assert int(re.search(r"VGPRs Spill: (\d+)", row).group(1)) == 0, row
