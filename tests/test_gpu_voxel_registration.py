"""Voxelised GICP on the GPU: Registration.align_voxel_map / Registration::align(source, map) over sp_vhm_prepare_registration,
sp_vhm_prepare_source, sp_vhm_linearize and sp_vhm_error (csrc/voxel_registration.hip), against the float64 model of
tests/f64_voxel_registration.py on its engineered scene (tests/test_voxel_registration_cpu.py holds the scene's conditions and the
model without a GPU) and, end to end, against the existing path: Registration.align on the map's export with a KD-tree.

  1. linearisation, 1 / 7 / 27 cells x GICP / POINT_TO_DISTRIBUTION x NONE / GEMAN_MCCLURE: voxel keys and inlier count exact,
     H, b, error within TOL_F64 per block, two runs bit-identical, pose on the host and on the device bit-identical
  2. the trial error over the frozen correspondences at a pose that moves every point by 0.6 cells
  3. the same map after one rehash (capacity 60013) and after remove_old_data took half of its cells
  3b. five voxels on ONE probe sequence (tests/voxel_chains.py): every one is found, at its own probe
  4. staleness and argument errors: code, message, nothing written
  5. end to end on three noisy planes, every optimiser, 1 and 7 cells, against the existing path and the known motion
  6. end to end on the bundled pair, LM + GEMAN_MCCLURE with the MAP prior and degenerate regularisation
  7. the C++ facade (tests/cpp/test_voxel_registration.cpp)

TOL_F64 = 2e-4 is the project's bound for a float32 kernel against float64 (tests/test_gpu_factors_f64.py).
Measured on an MI355X (`pytest -s` prints every figure before it is asserted): see MEASURED below."""
import os
import subprocess

import numpy as np
import pytest

import f64_factors as f64
import f64_voxel_registration as vr
from test_gpu_lidar_odometry import build

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CPP = os.path.join(ROOT, "tests", "cpp")
TOL_F64 = 2e-4
MODES, FACTORS, LOSSES = (1, 7, 27), ("GICP", "POINT_TO_DISTRIBUTION"), ("NONE", "GEMAN_MCCLURE")

MEASURED = """
Linearisation against float64 (worst block of H / half of b / error), inliers 110 / 219 / 235 of 288 with 1 / 7 / 27 cells, voxel keys
equal everywhere:      GICP + NONE 1.5e-5 (b, 1 cell)   GICP + GEMAN_MCCLURE 4.3e-6   POINT_TO_DISTRIBUTION 2.5e-6 (both losses)
  grown map 4.9e-6, after removal 3.1e-6 (7 cells, GICP, NONE, 121 inliers left)
  with the blob half of f64_factors.synthetic_covariances as source covariances (first draft of the scene): GICP + NONE 2.5e-4
  in b with 1 cell, 1.1e-4 with 27 — the float32 plane regulariser on near-isotropic matrices, see f64_voxel_registration.build_scene
Trial error over the frozen correspondences against float64: <= 8.8e-7; a fresh lookup at the trial pose would move 63 / 70 / 66 %.
Three planes (translation m, rotation rad against T_true; start 0.150, 0.0349):
  GN and LM   existing path 1.32e-3, 1.81e-4 | 1 cell 1.60e-3, 1.97e-4 | 7 cells 1.30e-3, 1.75e-4
  dog-leg     existing path 1.34e-3, 1.85e-4 | 1 cell 1.81e-3, 2.20e-4 | 7 cells 1.32e-3, 1.80e-4
  (planes ON voxel faces, first draft: 1 cell 2.49e-3, 2.80e-4 against 1.34e-3, 7.4e-5; 7 cells 1.23e-3, 7.0e-5)
Bundled pair, 6124 source points, 1073 voxels of 1 m (start 0.504, 0.0125): existing path 1.26e-2, 3.35e-3 in 8 iterations |
  voxel map 1.82e-2, 4.09e-3 in 10 iterations, 5381 inliers, 11 accepted of 11 evaluated LM trials.
C++ facade against align_voxel_map: the same bits in all three poses.
"""


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    from sycl_points_amd import _lib

    _lib.build()
    import sycl_points_amd.api as api

    return api


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cloud(sp, pts, covs=None):
    return sp.PointCloudShared(dev(np.asarray(pts, np.float32)), covs=None if covs is None else dev(np.asarray(covs, np.float32)))


def export_of(m):
    r = m.downsampling(distance=1e7)
    return vr.Export(r.points.cpu().numpy(), r.covs.cpu().numpy(), r.voxel_keys.cpu().numpy().view(np.uint64))


def scene_map(sp, scene, parts=1):
    m = sp.VoxelHashMap(vr.VOXEL_SIZE)
    m.set_min_num_point(vr.MIN_NUM_POINT)
    n = len(scene["tgt"])
    for a in range(parts):
        lo, hi = a * n // parts, (a + 1) * n // parts
        m.add_point_cloud(cloud(sp, scene["tgt"][lo:hi], scene["tcov"][lo:hi]))
    return m


def registration(sp, factor, loss="NONE", **kw):
    return sp.Registration(sp.RegistrationParams(reg_type=factor, robust_type=loss, max_correspondence_distance=vr.MAX_CORR, **kw))


class World:
    """the scene, its map on the device, the map's export, and the model's answers, each computed once"""

    def __init__(self, sp):
        self.sp = sp
        self.scene = vr.build_scene()
        self.map = scene_map(sp, self.scene)
        self.export = export_of(self.map)
        self.source = cloud(sp, self.scene["src"], self.scene["scov"])
        self._corr, self._case, self._ref = {}, {}, {}

    def corr(self, mode, pose="T", export=None):
        key = (mode, pose, id(export))
        if key not in self._corr:
            self._corr[key] = vr.correspondences(export or self.export, self.scene["src"], self.scene[pose], mode)
        return self._corr[key]

    def case(self, mode, export=None):
        key = (mode, id(export))
        if key not in self._case:
            nn, d2, _ = self.corr(mode, export=export)
            self._case[key] = vr.case_for(export or self.export, self.scene["src"], self.scene["scov"], self.scene["T"], nn, d2)
        return self._case[key]

    def ref(self, mode, factor, loss, export=None):
        key = (mode, factor, loss, id(export))
        if key not in self._ref:
            case = self.case(mode, export)
            s = vr.robust_scale(case, factor)
            self._ref[key] = (f64.system_fast(case, factor, loss, s), s)
        return self._ref[key]

    def prepared(self, factor, m=None):
        m = m or self.map
        if not m.registration_ready(factor):
            m.prepare_registration(factor)
        return m


@pytest.fixture(scope="module")
def world(sp):
    w = World(sp)
    bad, counts = vr.scene_report(w.scene, w.export)  # the conditions of the CPU test, on the device's own export
    assert not bad, bad[:10]
    return w


def lin_bytes(out):
    return bytes(out["lin"])[:176]


def check_linearisation(w, m, export, mode, factor, loss, tag):
    ref, s = w.ref(mode, factor, loss, export)
    _, _, keys = w.corr(mode, export=export)
    reg = registration(w.sp, factor, loss)
    out = reg.linearize_voxel_map(w.source, w.prepared(factor, m), w.scene["T"], s, mode, want_keys=True)
    got_keys = out["keys"].cpu().numpy().view(np.uint64)
    d = f64.distances(out["H"], out["b"], out["error"], ref)
    print(f"\n[voxel registration] {tag} cells {mode:2d} {factor:22s} {loss:14s} inlier {out['inlier']:3d} / {ref['inlier']:3d}  "
          f"keys differing {(got_keys != keys).sum()}  " + "  ".join(f"{k} {v:.1e}" for k, v in d.items()), end="")
    assert np.array_equal(got_keys, keys)
    assert out["inlier"] == ref["inlier"] and ref["inlier"] >= 50
    assert max(d.values()) <= TOL_F64, d
    again = reg.linearize_voxel_map(w.source, m, w.scene["T"], s, mode, want_keys=True)
    assert lin_bytes(again) == lin_bytes(out) and torch.equal(again["keys"], out["keys"])
    T_dev = dev(np.ascontiguousarray(w.scene["T"].T).reshape(-1))
    on_dev = reg.linearize_voxel_map(w.source, m, T_dev, s, mode)
    assert lin_bytes(on_dev) == lin_bytes(out)
    return reg, s


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("mode", MODES)
def test_linearisation_matches_float64_model(world, mode, factor, loss):
    check_linearisation(world, world.map, None, mode, factor, loss, "scene")


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("mode", MODES)
def test_frozen_trial_error(world, mode, factor, loss):
    w = world
    ref, s = w.ref(mode, factor, loss)
    nn, _, keys = w.corr(mode)
    _, _, fresh = w.corr(mode, "T_trial")
    moved = float((fresh[nn >= 0] != keys[nn >= 0]).mean())
    assert moved >= 0.5, moved  # a fresh lookup at the trial pose would pick other voxels: freezing is what is measured
    reg = registration(w.sp, factor, loss)
    m = w.prepared(factor)
    lin = reg.linearize_voxel_map(w.source, m, w.scene["T"], s, mode)
    want = f64.error_f64(w.case(mode), factor, loss, s, w.scene["T_trial"])
    err, inl = reg.error_voxel_map(w.source, m, w.scene["T_trial"], s)
    same, inl0 = reg.error_voxel_map(w.source, m, w.scene["T"], s)
    print(f"\n[voxel registration] trial cells {mode:2d} {factor:22s} {loss:14s} moved {moved:.2f}  error {err:.6g} / {want:.6g}  "
          f"rel {abs(err - want) / want:.1e}  at T: rel {abs(same - ref['error']) / ref['error']:.1e}", end="")
    assert inl == inl0 == lin["inlier"] == ref["inlier"]
    assert abs(err - want) <= TOL_F64 * want
    assert abs(same - ref["error"]) <= TOL_F64 * ref["error"]
    T_dev = dev(np.ascontiguousarray(w.scene["T_trial"].T).reshape(-1))
    assert reg.error_voxel_map(w.source, m, T_dev, s) == (err, inl)


def test_after_a_rehash(world):
    w = world
    m = w.sp.VoxelHashMap(vr.VOXEL_SIZE)
    m.set_min_num_point(vr.MIN_NUM_POINT)
    m.set_rehash_threshold(1e-4)
    n = len(w.scene["tgt"])
    for lo, hi in ((0, n // 2), (n // 2, n)):
        m.add_point_cloud(cloud(w.sp, w.scene["tgt"][lo:hi], w.scene["tcov"][lo:hi]))
    assert m.info("capacity") == 60013
    exp = export_of(m)
    assert set(exp.row) == set(w.export.row)
    m.prepare_registration("GICP")
    check_linearisation(w, m, exp, 7, "GICP", "NONE", "grown")
    # the rows follow a grow: prepared at 30029 slots, then grown, then prepared again
    m2 = w.sp.VoxelHashMap(vr.VOXEL_SIZE)
    m2.set_min_num_point(vr.MIN_NUM_POINT)
    m2.add_point_cloud(cloud(w.sp, w.scene["tgt"][:n // 2], w.scene["tcov"][:n // 2]))
    m2.prepare_registration("GICP")
    m2.set_rehash_threshold(1e-4)
    m2.add_point_cloud(cloud(w.sp, w.scene["tgt"][n // 2:], w.scene["tcov"][n // 2:]))
    assert m2.info("capacity") == 60013 and not m2.registration_ready("GICP")
    m2.prepare_registration("GICP")
    check_linearisation(w, m2, export_of(m2), 7, "GICP", "NONE", "prepared, grown, prepared")


def test_after_remove_old_data(world):
    w = world
    m = w.sp.VoxelHashMap(vr.VOXEL_SIZE)
    m.set_min_num_point(vr.MIN_NUM_POINT)
    m.set_max_staleness(2)
    m.set_remove_old_data_cycle(1)
    cells = np.floor(w.scene["tgt"][:, :3]).astype(np.int64)
    old = (cells.sum(axis=1) % 2) == 0  # half of the cells, a checkerboard
    m.add_point_cloud(cloud(w.sp, w.scene["tgt"][old], w.scene["tcov"][old]))
    before = m.info("voxel_num")
    for _ in range(2):
        m.add_point_cloud(w.sp.PointCloudShared())  # empty frames: the first half ages
    m.add_point_cloud(cloud(w.sp, w.scene["tgt"][~old], w.scene["tcov"][~old]))
    exp = export_of(m)
    kept = {tuple(c) for c in cells[~old]}
    assert 0 < before and m.info("voxel_num") == len(kept) and len(exp.keys) < len(w.export.keys)
    assert set(exp.row) == {k for k in w.export.row if k in {vr.key_of_cell(c) for c in kept}}
    m.prepare_registration("GICP")
    check_linearisation(w, m, exp, 7, "GICP", "NONE", "after removal")


def test_every_voxel_of_one_probe_sequence_is_found(sp):
    """Five keys that share their whole probe sequence at 30029 slots (tests/voxel_chains.py): the voxels sit at probes 0 .. 4, and a
    source point in each cell must find its own — the probes behind the first are a loop of their own in the kernel. The cells lie
    up to 2^20 cells from the origin, where a float32 coordinate resolves 1/16 of a cell: identity pose, dyadic coordinates, and
    only the exact outputs are held (keys, inlier count)."""
    import voxel_chains as vc

    keys = vc.chain(30029, 5, True, vc.NEIGHBOURS)
    assert len({vc.slot_id(k, 0, 30029) for k in keys}) == 1
    a, b = vc.points_of(keys, 1.0, 0.5), vc.points_of(keys, 1.0, 0.25)
    C3 = np.diag([0.01, 0.9, 1.1])
    covs = f64.cov16(np.broadcast_to(C3, (10, 3, 3)).astype(np.float32))
    m = sp.VoxelHashMap(1.0)
    m.set_min_num_point(2)
    for k in range(5):  # one key per frame: key k ends at probe k
        m.add_point_cloud(cloud(sp, np.concatenate([a[k:k + 1], b[k:k + 1]]), covs[:2]))
    assert m.info("voxel_num") == 5
    src = vc.points_of(keys, 1.0, 0.5)
    src[:, 0] += 0.25
    S = cloud(sp, src, covs[:5])
    m.prepare_registration("GICP")
    out = registration(sp, "GICP").linearize_voxel_map(S, m, np.eye(4, dtype=np.float32), neighbor_voxels=1, want_keys=True)
    assert out["inlier"] == 5
    assert np.array_equal(out["keys"].cpu().numpy().view(np.uint64), np.array(keys, np.uint64))
    assert np.isfinite(out["H"]).all() and out["error"] > 0.0


def test_staleness_and_arguments(world):
    w, sp = world, world.sp
    T, S = w.scene["T"], w.source
    n = S.size()

    def refused(code, text, call):
        lin = torch.full((48,), 7.0, dtype=torch.float32, device="cuda")
        with pytest.raises(sp.SpError) as e:
            call(lin)
        print(f"\n[voxel registration] refused ({e.value.code}): {e.value}", end="")
        assert e.value.code == code and text in str(e.value), (code, text, str(e.value))
        assert bool((lin == 7.0).all()), "a refused call wrote to its output"

    gicp, p2d = registration(sp, "GICP"), registration(sp, "POINT_TO_DISTRIBUTION")
    m = scene_map(sp, w.scene)
    not_ready = "call sp_vhm_prepare_registration"
    assert not m.registration_ready("GICP")
    refused(1, not_ready, lambda lin: gicp.linearize_voxel_map(S, m, T, lin=lin))  # before prepare
    m.prepare_registration("GICP")
    assert m.registration_ready("GICP") and not m.registration_ready("POINT_TO_DISTRIBUTION")
    refused(2, "no frozen correspondences", lambda lin: gicp.error_voxel_map(S, m, T, lin=lin))  # nothing linearised yet
    refused(1, not_ready, lambda lin: p2d.linearize_voxel_map(S, m, T, lin=lin))  # rows of the other factor
    ok = gicp.linearize_voxel_map(S, m, T)
    assert ok["inlier"] > 0 and gicp.error_voxel_map(S, m, T)[1] == ok["inlier"]
    need = sp._lib.lib().sp_vhm_registration_workspace_bytes(n)
    refused(1, "workspace too small", lambda lin: gicp.linearize_voxel_map(S, m, T, lin=lin, workspace_bytes=need - 1))
    refused(1, "workspace too small", lambda lin: gicp.error_voxel_map(S, m, T, lin=lin, workspace_bytes=need - 1))
    refused(1, "neighbor_voxels must be 1, 7 or 27", lambda lin: gicp.linearize_voxel_map(S, m, T, neighbor_voxels=5, lin=lin))
    refused(1, "reg_type must be GICP or POINT_TO_DISTRIBUTION",
            lambda lin: registration(sp, "POINT_TO_PLANE").linearize_voxel_map(S, m, T, lin=lin, prepare_source=False))
    refused(1, "rotation constraint",
            lambda lin: registration(sp, "GICP", rotation_constraint_enable=True).linearize_voxel_map(S, m, T, lin=lin))
    with pytest.raises(sp.SpError) as e:
        m.prepare_registration("POINT_TO_PLANE")
    assert e.value.code == 1 and "reg_type must be" in str(e.value)
    # everything that changes the table moves the generation: the rows and the frozen correspondences go stale
    other = registration(sp, "GICP")
    other.linearize_voxel_map(S, m, T)
    refused(2, "no frozen correspondences", lambda lin: gicp.error_voxel_map(S, m, T, lin=lin))  # another workspace came last
    gicp.linearize_voxel_map(S, m, T)
    for change in (lambda: m.add_point_cloud(cloud(sp, w.scene["tgt"][:5], w.scene["tcov"][:5])), lambda: m.set_min_num_point(3),
                   lambda: m.set_voxel_size(1.0), lambda: m.set_min_num_point(2)):
        change()
        assert not m.registration_ready("GICP")
        refused(1, not_ready, lambda lin: gicp.linearize_voxel_map(S, m, T, lin=lin))
        refused(1, not_ready, lambda lin: gicp.error_voxel_map(S, m, T, lin=lin))
        m.prepare_registration("GICP")
        refused(1, "changed since the linearisation", lambda lin: gicp.error_voxel_map(S, m, T, lin=lin))
        gicp.linearize_voxel_map(S, m, T)
        gicp.error_voxel_map(S, m, T)
    m.clear()
    assert not m.registration_ready("GICP")
    # a map built without covariances
    bare = sp.VoxelHashMap(vr.VOXEL_SIZE)
    bare.add_point_cloud(cloud(sp, w.scene["tgt"]))
    with pytest.raises(sp.SpError) as e:
        bare.prepare_registration("GICP")
    assert e.value.code == 1 and "no covariances" in str(e.value)
    refused(1, "no covariances", lambda lin: gicp.linearize_voxel_map(S, bare, T, lin=lin))
    # no source points: zero sums
    m2 = w.prepared("GICP")
    empty = sp.PointCloudShared(torch.zeros((0, 4), dtype=torch.float32, device="cuda"), covs=torch.zeros((0, 16), dtype=torch.float32, device="cuda"))
    lin = torch.full((48,), 7.0, dtype=torch.float32, device="cuda")
    out = gicp.linearize_voxel_map(empty, m2, T, lin=lin)
    assert out["inlier"] == 0 and out["error"] == 0.0 and not out["H"].any() and not out["b"].any()
    assert gicp.error_voxel_map(empty, m2, T) == (0.0, 0)
    assert np.array_equal(gicp.align_voxel_map(empty, m2, T).T, T)


# ------------------------------------------------------------------------------------------------ end to end
def pose_errors(T, T_true):
    T, T_true = np.asarray(T, np.float64), np.asarray(T_true, np.float64)
    dR = T[:3, :3] @ T_true[:3, :3].T
    # the angle from the skew part: acos of the trace resolves nothing below 3e-4 rad of a float32 rotation
    sin = 0.5 * np.linalg.norm([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    return float(np.linalg.norm(T[:3, 3] - T_true[:3, 3])), float(np.arctan2(sin, (np.trace(dR) - 1.0) / 2.0))


def with_covariances(sp, pts, k=10):
    c = sp.PointCloudShared(dev(pts))
    sp.covariance.estimate(sp.KDTree.build(c.points).knn_search(c.points, k), c)
    return c


def planes_scene(seed=5):
    """three orthogonal planes of 10 m x 10 m, 6700 points each, 1 cm of noise; the source: 2000 of them moved by T_true^-1
    (0.15 m, 2 degrees). The planes lie at x = 0.13, y = 0.21, z = 0.37: in general position to the 0.5 m voxels. (The first draft
    had them at 0, ON a voxel face: every plane's points then fall into two layers of voxels, each holding one half of the noise,
    and a lookup in the point's own cell alone flips between the two half-Gaussians; measured there: rotation error 2.8e-4 rad with 1
    cell against 7.4e-5 of the existing path and 7.0e-5 with 7 cells, translation 2.5e-3 / 1.3e-3 / 1.2e-3 m.)"""
    rs = np.random.RandomState(seed)
    pts = []
    for axis in range(3):
        p = rs.uniform(0.0, 10.0, (6700, 3))
        p[:, axis] = (0.13, 0.21, 0.37)[axis] + rs.normal(0.0, 0.01, 6700)
        pts.append(p)
    tgt = np.ones((20100, 4), np.float32)
    tgt[:, :3] = np.concatenate(pts)
    w = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0) * np.deg2rad(2.0)
    t = np.array([0.1, -0.08, 0.08])
    t *= 0.15 / np.linalg.norm(t)
    from scipy.linalg import expm

    T_true = expm(f64.twist_matrix(np.concatenate([w, np.zeros(3)])))
    T_true[:3, 3] = t
    Ti = np.linalg.inv(T_true)
    pick = rs.permutation(len(tgt))[:2000]
    src = np.ones((2000, 4), np.float32)
    src[:, :3] = tgt[pick, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]
    return tgt, src, T_true


@pytest.fixture(scope="module")
def planes(sp):
    tgt, src, T_true = planes_scene()
    target, source = with_covariances(sp, tgt), with_covariances(sp, src)
    m = sp.VoxelHashMap(0.5)
    m.add_point_cloud(target)
    means = m.downsampling(distance=1e7)
    return {"map": m, "source": source, "means": means, "tree": sp.KDTree.build(means.points), "T_true": T_true}


def end_to_end_params(sp, method, **kw):
    return sp.RegistrationParams(reg_type="GICP", optimization_method=method, max_correspondence_distance=1.0, max_iterations=30,
                                 criteria_translation=1e-5, criteria_rotation=1e-5, **kw)


@pytest.mark.parametrize("method", ["GN", "LM", "DOGLEG"])
def test_end_to_end_planes(sp, planes, method):
    """Measured on an MI355X, (translation error m, rotation error rad) against T_true; reference = Registration.align on the
    map's export with a KD-tree: see MEASURED."""
    p = planes
    ref = sp.Registration(end_to_end_params(sp, method)).align(p["source"], p["means"], p["tree"])
    rt, rr = pose_errors(ref.T, p["T_true"])
    start = pose_errors(np.eye(4), p["T_true"])
    print(f"\n[voxel registration] planes {method}: start {start[0]:.4f} m {start[1]:.5f} rad | existing path {rt:.2e} m {rr:.2e} rad "
          f"({ref.iterations} iterations, {ref.inlier} inliers)", end="")
    assert rt < 0.1 * start[0] and rr < 0.1 * start[1]  # the reference itself has found the motion
    for cells in (1, 7):
        got = sp.Registration(end_to_end_params(sp, method)).align_voxel_map(p["source"], p["map"], neighbor_voxels=cells)
        vt, vrot = pose_errors(got.T, p["T_true"])
        print(f" | {cells} cells {vt:.2e} m {vrot:.2e} rad ({got.iterations} iterations, {got.inlier} inliers)", end="")
        assert vt <= 2.0 * rt and vrot <= 2.0 * rr, (method, cells, (vt, vrot), (rt, rr))


def test_end_to_end_bundled_pair(sp):
    """tests/golden: box filter, voxel grid 0.25, k = 10 covariances (the reference's example); the target accumulated into a map of
    1 m voxels. LM + GEMAN_MCCLURE, degenerate regularisation and the MAP prior on (the prior from a previous frame's alignment
    that ended at the identity, the prediction the identity). Measured: see MEASURED."""
    from test_gpu_facade import read_ply_xyz

    def prep(name):
        pts = dev(read_ply_xyz(os.path.join(GOLD, name)))
        pts = sp.compact_by_flags(pts, sp.box_filter_flags(pts, 0.5, 50.0)).contiguous()
        c = sp.VoxelGrid(0.25).downsampling(sp.PointCloudShared(pts))
        return with_covariances(sp, c.points.contiguous().cpu().numpy())

    source, target = prep("source.ply"), prep("target.ply")
    T_gt = np.loadtxt(os.path.join(GOLD, "T_target_source.txt"))
    m = sp.VoxelHashMap(1.0)
    m.add_point_cloud(target)
    means = m.downsampling(distance=1e7)
    tree = sp.KDTree.build(means.points)
    kw = dict(robust_type="GEMAN_MCCLURE", robust_default_scale=2.5, degenerate_reg_type="NL_REG", map_prior_enabled=True)
    params = lambda: sp.RegistrationParams(reg_type="GICP", optimization_method="LM", max_correspondence_distance=2.0,  # noqa: E731
                                           max_iterations=30, **kw)
    prev = sp.Registration(sp.RegistrationParams(max_iterations=1, max_correspondence_distance=2.0)).align(source, means, tree)
    prev.T = np.eye(4, dtype=np.float32)  # the previous frame ended here; its raw system weighs the prior
    ref_reg, reg = sp.Registration(params()), sp.Registration(params())
    assert ref_reg.set_map_prior_state(prev, np.eye(4, dtype=np.float32)) and reg.set_map_prior_state(prev, np.eye(4, dtype=np.float32))
    ref = ref_reg.align(source, means, tree)
    got = reg.align_voxel_map(source, m)
    (rt, rr), (vt, vrot) = pose_errors(ref.T, T_gt), pose_errors(got.T, T_gt)
    start = pose_errors(np.eye(4), T_gt)
    accepted, trials = sum(e["accepted"] for e in got.log), sum(e["trials"] for e in got.log)
    print(f"\n[voxel registration] bundled pair, {source.size()} source points, {means.size()} voxels: start {start[0]:.3f} m "
          f"{start[1]:.4f} rad | existing path {rt:.3e} m {rr:.3e} rad ({ref.iterations} it) | voxel map {vt:.3e} m {vrot:.3e} rad "
          f"({got.iterations} it, {got.inlier} inliers, {accepted} accepted, {trials} trials)")
    assert accepted >= 1 and trials >= 1
    assert np.trace(got.H - got.H_raw) > 0.0  # the host-side pose terms are in the system the optimiser solved
    assert vt <= 2.0 * rt and vrot <= 2.0 * rr, ((vt, vrot), (rt, rr))


def test_cpp_facade(sp, planes, tmp_path):
    """Registration::align(source, map) of the C++ facade against align_voxel_map, bit for bit. The target both sides build their
    map from is the EXPORT of the planes scene's map (its voxel means and covariances, one point per voxel): a map accumulates
    with float atomics, whose order is not fixed, so two maps built from the 20 100 points need not agree in the last bit; one
    point per voxel and frame adds nothing to anything. The second frame (the export again) makes the map change under the
    C++ object, which has to refresh the rows by itself."""
    exe = build(os.path.join(CPP, "test_voxel_registration.cpp"), os.path.join(CPP, "test_voxel_registration"))
    p = planes
    tp, tc = p["means"].points.cpu().numpy(), p["means"].covs.cpu().numpy()
    spn, sc = p["source"].points.cpu().numpy(), p["source"].covs.cpu().numpy()
    path = str(tmp_path / "planes.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(tp), len(spn)], np.int32).tobytes())
        for a in (tp, tc, spn, sc):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout[-4000:]
    theirs = {}
    for line in r.stdout.splitlines():
        if line.startswith("T "):
            name, *words = line[2:].split()
            theirs[name] = np.array([int(x, 16) for x in words], np.uint32).view(np.float32).reshape(4, 4).T
    m = sp.VoxelHashMap(0.5)
    target = cloud(sp, tp, tc)
    m.add_point_cloud(target)
    mine = {}
    for name, method, cells in (("gn1", "GN", 1), ("lm7", "LM", 7)):
        mine[name] = sp.Registration(end_to_end_params(sp, method)).align_voxel_map(p["source"], m, neighbor_voxels=cells).T
    reg = sp.Registration(end_to_end_params(sp, "GN"))
    reg.align_voxel_map(p["source"], m)
    m.add_point_cloud(target)
    mine["gn1_second_frame"] = reg.align_voxel_map(p["source"], m).T
    assert set(theirs) == set(mine)
    for name in mine:
        d = np.abs(theirs[name] - mine[name]).max()
        print(f"[voxel registration] C++ against Python, {name}: max |dT| = {d:.3g}; against T_true {pose_errors(mine[name], p['T_true'])}")
        assert np.array_equal(theirs[name].view(np.uint32), np.asarray(mine[name], np.float32).view(np.uint32)), name
