"""A float64 model of voxelised GICP (sp_vhm_linearize / sp_vhm_error: a scan linearised against a VoxelHashMap), written from the
mathematics, and the engineered scene its tests share. A plain helper module for tests/test_voxel_registration_cpu.py (scene
conditions, model against finite differences; the map is the oracle's) and tests/test_gpu_voxel_registration.py (the kernels).

The correspondence of a source point p at pose T:
    q = T p;   c = floor(q / size) per axis;   probed cells c + d, d from 1, 7 (|d|_1 <= 1) or 27 (|d|_inf <= 1) offsets;
    a probed cell counts when each of its indices lies in [-2^20, 2^20) and the map EXPORTS a voxel with its key — the export
    (VoxelHashMap.downsampling() with its voxel_keys) lists the voxels with at least min_num_point points, their means and their
    covariances (exp of the mean log-covariance). Means and covariances are taken from that export, never recomputed here;
    among the cells that count the one whose mean is nearest to q wins; no correspondence when |q - mean|^2 > max_corr^2, when q is
    not finite, when no cell counts.
The linearised system over these correspondences is f64_factors' (system_fast / system_fd / error_f64) for GICP and
POINT_TO_DISTRIBUTION with the voxel means as target points and the voxel covariances as target covariances.

build_scene() draws the engineered scene (voxel 1.0, min_num_point 2, max_correspondence_distance 0.6) and redraws every source
point that violates a condition of scene_report(); the tests assert that report on the map they use."""
import itertools

import numpy as np
from scipy.linalg import expm

import f64_factors as f64

VOXEL_SIZE, MIN_NUM_POINT, MAX_CORR = 1.0, 2, 0.6
INVALID_KEY = (1 << 64) - 1
FIELD_BITS, FIELD_OFFSET = 21, 1 << 20
CLASSES = ("own", "face", "edge_corner", "nothing", "single", "far_mean", "nan", "out_of_range")
MIN_PER_CLASS = 8
FACE_MARGIN, REL_MARGIN = 0.02, 1e-3
TRIAL_SHIFT = np.array([0.6, 0.0, 0.0])  # |shift| = 0.6 cells


def offsets(mode, _cache={}):
    """the probed cells of a mode as a set of offsets (the model needs no order: the scene has no ties)"""
    if mode not in _cache:
        _cache[mode] = _offsets(mode)
    return _cache[mode]


def _offsets(mode):
    all27 = [d for d in itertools.product((-1, 0, 1), repeat=3)]
    if mode == 1:
        return [(0, 0, 0)]
    if mode == 7:
        return [d for d in all27 if sum(abs(x) for x in d) <= 1]
    if mode == 27:
        return all27
    raise ValueError(mode)


def key_of_cell(cell):
    f = [int(c) + FIELD_OFFSET for c in cell]
    if not all(0 <= x < (1 << FIELD_BITS) for x in f):
        return INVALID_KEY
    return f[0] | (f[1] << FIELD_BITS) | (f[2] << (2 * FIELD_BITS))


class Export:
    """points (n, 4) float32, covs (n, 16) float32, keys (n,) uint64 of a map's downsampling(), as numpy arrays"""

    def __init__(self, points, covs, keys):
        self.points = np.asarray(points, np.float32).reshape(-1, 4)
        self.covs = np.asarray(covs, np.float32).reshape(-1, 16)
        self.keys = np.asarray(keys).astype(np.uint64)
        self.row = {int(k): i for i, k in enumerate(self.keys)}
        assert len(self.row) == len(self.keys), "a key exported twice"
        self.means = self.points[:, :3].astype(np.float64)


def transform(T, p):
    T = np.asarray(T, np.float64)
    with np.errstate(invalid="ignore"):
        return np.asarray(p, np.float32)[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]


def candidates(export, q, mode, size=VOXEL_SIZE):
    """(row in the export, squared distance) of every probed cell of q that counts"""
    if not np.isfinite(q).all():
        return []
    c = np.floor(q / size)
    out = []
    for d in offsets(mode):
        k = key_of_cell((c[0] + d[0], c[1] + d[1], c[2] + d[2]))
        r = export.row.get(k) if k != INVALID_KEY else None
        if r is not None:
            out.append((r, float(((q - export.means[r]) ** 2).sum())))
    return out


def correspondences(export, src, T, mode, max_corr=MAX_CORR, size=VOXEL_SIZE):
    """nn (row in the export, -1: none), d2 (float32; f64_factors.REJECTED_D2 for none), keys (uint64, INVALID_KEY for none)"""
    Q = transform(T, src)
    nn = np.full(len(src), -1, np.int64)
    d2 = np.full(len(src), f64.REJECTED_D2, np.float64)
    for i, q in enumerate(Q):
        cand = candidates(export, q, mode, size)
        if cand:
            r, d = min(cand, key=lambda x: x[1])
            if d <= max_corr * max_corr:
                nn[i], d2[i] = r, d
    keys = np.full(len(src), INVALID_KEY, np.uint64)
    keys[nn >= 0] = export.keys[nn[nn >= 0]]
    return nn, d2.astype(np.float32), keys


def case_for(export, src, scov, T, nn, d2, max_corr=MAX_CORR):
    """the f64_factors case of these correspondences: voxel means as target points, voxel covariances as target covariances"""
    nrm = np.zeros((len(export.points), 4), np.float32)
    c = f64.Case(np.asarray(src, np.float32), np.asarray(scov, np.float32), export.points, export.covs, nrm,
                 np.maximum(nn, 0).astype(np.int32), np.asarray(d2, np.float32), np.asarray(T, np.float32))
    c.max_corr = max_corr
    assert np.array_equal(c.inliers, nn >= 0)
    return c


def robust_scale(case, factor):
    """the float32-rounded median residual norm of the inliers: both sides of the scale are populated"""
    return float(np.float32(np.median(f64.residual_norms(case, factor))))


# ---- the engineered scene
BLOCK_ORIGIN, BLOCK_SHAPE = np.array([2, -3, 0]), (6, 6, 3)


def _rotation_jitter(rs, angle):
    w = rs.normal(size=3)
    w *= angle / np.linalg.norm(w)
    return expm(f64.twist_matrix(np.concatenate([w, np.zeros(3)])))[:3, :3]


def build_target(rs):
    """About 60 occupied cells of the 6 x 6 x 3 block, 1 to 5 points each in the inner [0.2, 0.8]^3 of their cell; the points of a
    cell share one planar covariance shape (eigenvalues (0.01, 0.9, 1.1) x a scale in [1, 2], one rotation per cell, per-point
    jitter of 3 % per eigenvalue and 0.01 rad). Every seventh occupied cell holds a single point (below min_num_point).
    The two large eigenvalues are kept 20 % apart on purpose: next to a DOUBLE eigenvalue the analytic fp32 eigen-solver that map
    and oracle share (symmetric_eigen3; tests/f64_features.py describes the spot) returns eigenvectors that are orthogonal to 1e-3
    only, and the log-Euclidean mean of such a cell came out with a smallest eigenvalue of 2e-6 instead of 1.2e-2 when they were
    3 % apart. That is the map's business, not this feature's; scene_report holds every exported covariance to a clear gap and to
    a determinant far from eigen_utils::inverse's 1e-6."""
    cells = [BLOCK_ORIGIN + np.array(ijk) for ijk in itertools.product(*(range(s) for s in BLOCK_SHAPE))]
    chosen = rs.permutation(len(cells))[:60]
    pts, covs, counts = [], [], {}
    V_cell = f64.random_rotations(rs, len(chosen))
    for n, ci in enumerate(chosen):
        cell = cells[ci]
        m = 1 if n % 7 == 3 else int(rs.randint(2, 6))
        counts[tuple(int(x) for x in cell)] = m
        scale = rs.uniform(1.0, 2.0)
        for _ in range(m):
            pts.append(cell + rs.uniform(0.2, 0.8, 3))
            lam = np.array([0.01, 0.9, 1.1]) * scale * (1.0 + rs.uniform(-0.03, 0.03, 3))
            V = _rotation_jitter(rs, 0.01) @ V_cell[n]
            C = V @ np.diag(lam) @ V.T
            covs.append(0.5 * (C + C.T))
    P = np.ones((len(pts), 4), np.float32)
    P[:, :3] = np.array(pts)
    return P, f64.cov16(np.array(covs).astype(np.float32)), counts


def classify(q, counts):
    """the class of a finite q from the occupancy alone (counts: cell -> number of points)"""
    c = tuple(int(x) for x in np.floor(q / VOXEL_SIZE))
    if any(not (-FIELD_OFFSET <= x < FIELD_OFFSET) for x in c):
        return "out_of_range"
    valid = lambda d: counts.get((c[0] + d[0], c[1] + d[1], c[2] + d[2]), 0) >= MIN_NUM_POINT  # noqa: E731
    own = counts.get(c, 0)
    if own >= MIN_NUM_POINT:
        return "own"  # ("far_mean" is told apart by the distance to the mean, below)
    if own == 1:
        return "single"
    if any(valid(d) for d in offsets(7)):
        return "face"
    if any(valid(d) for d in offsets(27)):
        return "edge_corner"
    return "nothing"


def _point_ok(means_by_cell, q):
    """the per-point conditions at one pose: the face margin, best against second best, every candidate against max_corr^2"""
    if not np.isfinite(q).all():
        return True
    fr = q / VOXEL_SIZE - np.floor(q / VOXEL_SIZE)
    if (fr < FACE_MARGIN).any() or (fr > 1.0 - FACE_MARGIN).any():
        return False
    c = np.floor(q / VOXEL_SIZE)
    for mode in (1, 7, 27):
        d = sorted(float(((q - means_by_cell[k]) ** 2).sum())
                   for k in ((c[0] + o[0], c[1] + o[1], c[2] + o[2]) for o in offsets(mode)) if k in means_by_cell)
        if len(d) > 1 and (d[1] - d[0]) < REL_MARGIN * d[1]:
            return False
        if any(abs(x - MAX_CORR ** 2) < REL_MARGIN * MAX_CORR ** 2 for x in d):
            return False
    return True


def build_scene(seed=20250917):
    """target points / covariances, about 300 source points built backwards as p = T^-1 q with T from f64_factors.GENERATING_TWIST,
    source covariances, T (float32), the trial pose (every point shifted by 0.6 cells) and each source point's class. A candidate q
    that violates a condition at T or at the trial pose (on the float32-rounded p) is drawn again. The first half of the face
    class and of the edge / corner class is drawn next to a voxel mean, so that it has a neighbour's mean within
    max_correspondence_distance: what 7 cells reach and 1 does not, what 27 reach and 7 do not."""
    rs = np.random.RandomState(seed)
    tgt, tcov, counts = build_target(rs)
    # the drawing aid: float64 means of the cells that count (the tests check the conditions on the map's own export)
    sums = {}
    for p in tgt[:, :3].astype(np.float64):
        sums.setdefault(tuple(int(x) for x in np.floor(p / VOXEL_SIZE)), []).append(p)
    means = {k: np.mean(v, axis=0) for k, v in sums.items() if len(v) >= MIN_NUM_POINT}
    T = expm(f64.twist_matrix(f64.GENERATING_TWIST)).astype(np.float32)
    Tt = T.astype(np.float64).copy()
    Tt[:3, 3] += TRIAL_SHIFT
    Tt = Tt.astype(np.float32)
    Tinv = np.linalg.inv(T.astype(np.float64))
    quota = {"own": 110, "face": 50, "edge_corner": 30, "nothing": 20, "single": 30, "far_mean": 30, "nan": 8, "out_of_range": 10}
    have = {k: 0 for k in quota}
    src, classes = [], []
    lo, hi = BLOCK_ORIGIN - 2.0, BLOCK_ORIGIN + np.array(BLOCK_SHAPE) + 2.0
    mean_list = [means[k] for k in sorted(means)]
    near = lambda q, mode: any(d <= MAX_CORR ** 2 for d in (  # noqa: E731
        ((q - means[k]) ** 2).sum() for k in (tuple(int(x) for x in np.floor(q) + np.array(o)) for o in offsets(mode)) if k in means))
    while any(have[k] < quota[k] for k in quota):
        kind = None
        if have["nan"] < quota["nan"]:
            kind = "nan"
        elif have["out_of_range"] < quota["out_of_range"]:
            kind = "out_of_range"
        q = rs.uniform(lo, hi)
        want_near = kind is None and (have["face"] < quota["face"] // 2 or have["edge_corner"] < quota["edge_corner"] // 2)
        if want_near:
            v = rs.normal(size=3)
            q = mean_list[rs.randint(len(mean_list))] + v / np.linalg.norm(v) * rs.uniform(0.25, 0.58)
        if kind == "out_of_range":
            q[have[kind] % 3] = (1.5e6 + rs.uniform(0, 1000.0)) * (1 if have[kind] % 2 else -1)
        p = np.ones(4, np.float32)
        p[:3] = Tinv[:3, :3] @ q + Tinv[:3, 3]
        if kind == "nan":
            p[have[kind] % 3] = np.nan
        q1, q2 = transform(T, p[None])[0], transform(Tt, p[None])[0]
        if kind is None:
            kind = classify(q1, counts)
            if kind == "own" and ((q1 - means[tuple(int(x) for x in np.floor(q1))]) ** 2).sum() > MAX_CORR ** 2:
                kind = "far_mean"
            if kind in ("nan", "out_of_range") or have[kind] >= quota[kind]:
                continue
            if kind in ("face", "edge_corner") and have[kind] < quota[kind] // 2 and not near(q1, 7 if kind == "face" else 27):
                continue
        elif kind == "out_of_range" and classify(q1, counts) != "out_of_range":
            continue
        if not (_point_ok(means, q1) and _point_ok(means, q2)):
            continue
        have[kind] += 1
        src.append(p)
        classes.append(kind)
    order = rs.permutation(len(src))  # the classes interleaved: every wave sees several
    src = np.array(src, np.float32)[order]
    classes = [classes[i] for i in order]
    # Source covariances: the planar family of f64_factors.synthetic_covariances alone (eigenvalues 0.004 : 0.09 : 0.15), what a
    # k-NN covariance on a scanned surface looks like. Its blobs (1 : 1.18 : 1.36) are left out: GICP's plane() keeps only the
    # DIRECTION of the smallest eigenvalue, which rounding moves by eps / gap, and with the blobs the float32 regulariser every
    # GICP kernel shares (plane_regularize; tests/test_gpu_features_f64.py is its test) alone moves this scene's b by 2.5e-4 of
    # its size against float64 plane() — measured on the CPU with the oracle's update_covariance_plane in the model's place,
    # everything else float64; the target's share is 5e-6. The per-point algebra on blobs is tests/test_gpu_factors_f64.py's.
    Cs = f64.synthetic_covariances(rs, 2 * len(src))[0][0::2]
    return {"tgt": tgt, "tcov": tcov, "counts": counts, "src": src, "scov": f64.cov16(Cs), "T": T, "T_trial": Tt, "classes": classes}


def scene_report(scene, export):
    """What the tests assert of the scene on the map they use: a list of violated conditions (empty when all hold) and the class
    counts. Float64 on the float32-rounded inputs, at T and at the trial pose."""
    bad = []
    means = {}
    for k, r in export.row.items():
        cell = tuple(((k >> (FIELD_BITS * a)) & ((1 << FIELD_BITS) - 1)) - FIELD_OFFSET for a in range(3))
        means[cell] = export.means[r]
    valid_cells = {c for c, m in scene["counts"].items() if m >= MIN_NUM_POINT}
    if set(means) != valid_cells:
        bad.append("the export does not list exactly the cells with min_num_point points")
    for name, T in (("T", scene["T"]), ("T_trial", scene["T_trial"])):
        for i, q in enumerate(transform(T, scene["src"])):
            if not _point_ok(means, q):
                bad.append(f"source {i} at {name}: face margin, best / second best or max_corr margin")
    lam = np.linalg.eigvalsh(f64.cov3(export.covs))
    if not (lam[:, 0] <= 0.5 * lam[:, 1]).all():
        bad.append("an exported covariance without a clear smallest eigenvalue")
    if not (np.linalg.det(f64.cov3(export.covs)) >= 4e-6).all():
        bad.append("an exported covariance too close to eigen_utils::inverse's 1e-6")
    counts = {k: 0 for k in CLASSES}
    for i, q in enumerate(transform(scene["T"], scene["src"])):
        if not np.isfinite(q).all():
            kind = "nan"
        else:
            kind = classify(q, scene["counts"])
            if kind == "own" and ((q - means[tuple(int(x) for x in np.floor(q))]) ** 2).sum() > MAX_CORR ** 2:
                kind = "far_mean"
        counts[kind] += 1
        if kind != scene["classes"][i]:
            bad.append(f"source {i} is of class {kind}, drawn as {scene['classes'][i]}")
    for k in CLASSES:
        if counts[k] < MIN_PER_CLASS:
            bad.append(f"class {k}: {counts[k]} points")
    return bad, counts
