"""Global registration on the device (csrc/global_registration.hip) against the float64 model of tests/f64_fpfh.py.

  1. SPFH counts: equal to the model's wherever the model is sure. A pair is uncertain when a scaled feature lies within 1e-4 of
     an integer or |v| < 1e-3 dist (float64); rows without one: counts and m equal; other rows: the L1 difference of each group
     of 11 counts <= 2 x the row's uncertain pairs; at most 1 % of all pairs uncertain.
  2. FPFH rows against the model fed the device's own counts: every bin within 1e-3 on the 0..100 scale (a chain of at most
     64 + 15 float32 operations on values <= 100: 79 x 2^-24 x 100 = 4.7e-4); the three pad floats exactly 0.
  3. The match: first identity rows against an asymmetric integer B (exact in float32: index and distance equal), then with
     bound(i, j) = 40 x 2^-24 x (|a_i|^2 + |b_j|^2): the returned index lies within 2 bound of the float64 minimum, the returned
     distance within bound of that index's float64 distance, duplicate rows give the lowest index; mutual pairs equal to the
     model's wherever no decision lies inside the bound, at most 2 % of the rows excused (differing, with such a decision),
     ascending. On the bundled pair the rows WITH a decision inside the bound are 2.8 % (30 of 1 064 on the model's own
     descriptors): the scans' planar patches have descriptors of |f|^2 = 28 000, so bound = 0.13 against gaps of 0.002 .. 0.27
     between their nearest and second-nearest rows. No implementation changes that figure, so the 2 % is held against the rows
     that are in fact excused; measured on an MI355X: 139 pairs on both sides, 3 rows differ, each among the 29 of 1 065 rows
     (2.7 %) with such a decision.
  4. Scores: a hypothesis with a gate quantity within relative 1e-4 of its threshold is excused (at most 1 % of them); otherwise
     |score - model| <= the number of matches whose float64 residual lies within delta = 64 x 2^-24 x E / 0.2 of tau, E the
     largest absolute coordinate plus tau, 0.2 the triangle gate.
  5. End to end on the bundled pair with the source turned by 150 degrees: align from the identity ends more than 1 rad from
     the truth; align_global ends within twice the errors of align_batch started at the truth; two runs give the same bytes; an
     empty source and descriptors of a single plane return converged == False. Measured: align from the identity ends 2.47 rad
     off; align_batch from the truth 4.24e-2 m / 1.02e-2 rad, align_global 4.28e-2 m / 1.03e-2 rad, all 64 guesses within
     0.1 rad / 1 m of the truth.
  6. The C++ facade (tests/cpp/test_global_registration.cpp): descriptors, guesses and winner are the Python mirror's bits.
`pytest -s` prints every figure before it is asserted."""
import os

import numpy as np
import pytest

import f64_fpfh as model

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FLT_MAX = float(np.finfo(np.float32).max)
U = 2.0 ** -24


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


def cloud_of(sp, xyz, normals):
    p = np.ones((len(xyz), 4), np.float32)
    p[:, :3] = xyz
    n = np.zeros((len(xyz), 4), np.float32)
    n[:, :3] = normals
    return sp.PointCloudShared(dev(p), normals=dev(n))


def knn_of(sp, idx, d2):
    return sp.KNNResult(indices=dev(idx, np.int32), distances=dev(d2, np.float32), query_size=idx.shape[0], k=idx.shape[1])


# ----------------------------------------------------------------------------------------------------------- the bundled pair
@pytest.fixture(scope="module")
def bundled(sp):
    """The bundled scans at 1 m voxels on the device: box filter, voxel grid, the source turned by 150 degrees about z around the
    sensor, 20-NN lists, 10-NN normals turned towards the sensor, covariances, FPFH rows."""
    T = np.loadtxt(os.path.join(GOLD, "T_target_source.txt"))
    Rz = model.rot_z(150.0)
    out = {"T_true": T @ np.linalg.inv(Rz)}
    for name in ("source", "target"):
        pts = dev(model.read_ply_xyz(os.path.join(GOLD, name + ".ply")))
        pts = sp.compact_by_flags(pts, sp.box_filter_flags(pts, 0.5, 50.0)).contiguous()
        xyz = sp.VoxelGrid(1.0).downsampling(sp.PointCloudShared(pts)).points.contiguous().cpu().numpy()
        if name == "source":
            xyz[:, :3] = (xyz[:, :3].astype(np.float64) @ Rz[:3, :3].T).astype(np.float32)
        xyz[:, 3] = 1.0
        c = sp.PointCloudShared(dev(xyz))
        tree = sp.KDTree.build(c.points)
        knn = tree.knn_search(c, 20)
        nrm = sp.covariance.estimate_normals(tree.knn_search(c, 10), c)
        away = (nrm[:, :3] * c.points[:, :3]).sum(1, keepdim=True) > 0  # towards the sensor, every one of them
        c.normals = torch.where(away, -nrm, nrm).contiguous()
        sp.covariance.estimate(knn, c)
        out[name] = dict(cloud=c, tree=tree, knn=knn, fpfh=sp.fpfh(knn, c), xyz=xyz[:, :3].astype(np.float64),
                         normals=c.normals.cpu().numpy()[:, :3].astype(np.float64), idx=knn.indices.cpu().numpy(),
                         d2=knn.distances.cpu().numpy())
    return out


# --------------------------------------------------------------------------------------------------------------- 1, 2. FPFH
def random_cloud(n, seed, spread=3.0):
    rs = np.random.RandomState(seed)
    xyz = rs.uniform(-spread, spread, (n, 3)).astype(np.float32).astype(np.float64)
    nrm = rs.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return xyz, nrm.astype(np.float32).astype(np.float64)


def lists(xyz, k, drop_self=False):
    idx, d2 = model.knn_self(xyz, k + (1 if drop_self else 0))
    if drop_self:
        idx, d2 = idx[:, 1:], d2[:, 1:]
    return np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(d2.astype(np.float32))


def fpfh_case(name, bundled):
    if name == "n1":
        xyz, nrm = random_cloud(1, 1)
        return xyz, nrm, np.zeros((1, 1), np.int32), np.zeros((1, 1), np.float32)
    if name in ("n2", "n65"):
        n = int(name[1:])
        xyz, nrm = random_cloud(n, n)
        return (xyz, nrm) + lists(xyz, min(20, n))
    if name in ("k1", "k20", "k64"):
        xyz, nrm = random_cloud(200, 5)
        return (xyz, nrm) + lists(xyz, int(name[1:]), drop_self=name == "k1")  # (k = 1: the one entry is a neighbour)
    if name == "radius":  # a radius search: lists of different lengths, padded
        xyz, nrm = random_cloud(300, 6)
        idx, d2 = lists(xyz, 20)
        far = d2 > 1.0
        idx[far], d2[far] = -1, FLT_MAX
        assert far.any() and (~far[:, 1:]).any() and far[:, 1:].all(1).any()  # (some rows are left without a neighbour)
        return xyz, nrm, idx, d2
    if name == "no_self":
        xyz, nrm = random_cloud(130, 7)
        return (xyz, nrm) + lists(xyz, 20, drop_self=True)
    if name == "duplicates":
        xyz, nrm = random_cloud(150, 8)
        xyz[10:20] = xyz[0:10]  # the same place twice: dist == 0, skipped, still a neighbour
        xyz[40] = xyz[41] = xyz[42]
        return (xyz, nrm) + lists(xyz, 20)
    if name == "nan_normal":
        xyz, nrm = random_cloud(150, 9)
        nrm[3] = np.nan
        nrm[77, 1] = np.nan
        return (xyz, nrm) + lists(xyz, 20)
    assert name == "bundled_target"
    t = bundled["target"]
    return t["xyz"], t["normals"], t["idx"], t["d2"]


FPFH_CASES = ("n1", "n2", "n65", "k1", "k20", "k64", "radius", "no_self", "duplicates", "nan_normal", "bundled_target")


@pytest.mark.parametrize("name", FPFH_CASES)
def test_spfh_counts_and_fpfh_rows(sp, bundled, name):
    xyz, nrm, idx, d2 = fpfh_case(name, bundled)
    n, k = idx.shape
    rows, counts, m = sp.fpfh(knn_of(sp, idx, d2), cloud_of(sp, xyz, nrm), want_counts=True)
    rows, counts, m = rows.cpu().numpy(), counts.cpu().numpy().astype(np.int64), m.cpu().numpy().astype(np.int64)
    # the model reads what the device read: float32 points and normals
    want, want_m, unsure, pairs = model.spfh_counts(xyz.astype(np.float32), nrm.astype(np.float32), idx)
    total_unsure, total_pairs = int(unsure.sum()), int(pairs.sum())
    sure = unsure == 0
    l1 = np.abs(counts - want).reshape(n, 3, 11).sum(2)
    print(f"\n[spfh {name}] n {n} k {k}: {total_pairs} pairs, {total_unsure} uncertain, rows with a difference "
          f"{int((l1.sum(1) > 0).sum())}, largest L1 {int(l1.max()) if n else 0}", end="")
    assert np.array_equal(m, want_m)
    assert np.array_equal(counts[sure], want[sure])
    assert (l1 <= 2 * unsure[:, None]).all()
    assert total_unsure <= 0.01 * max(total_pairs, 1)
    if name == "n1":
        assert m[0] == 0 and not counts.any() and not rows.any()
    # 2. the rows from the device's own counts
    ref = model.fpfh_from_counts(counts, m, idx, d2)
    err = np.abs(rows[:, :33] - ref).max() if n else 0.0
    sums = rows[:, :33].reshape(n, 3, 11).sum(2)
    print(f" | fpfh: max |row - model| {err:.2e}, group sums in [{sums.min():.4f}, {sums.max():.4f}]")
    assert np.isfinite(rows).all() and err <= 1e-3
    assert not rows[:, 33:].any() and rows.shape == (n, 36)
    assert (np.abs(sums - 100.0) < 1e-2)[ref.reshape(n, 3, 11).sum(2) > 0].all()


def test_fpfh_is_reproducible(sp, bundled):
    t = bundled["target"]
    again = sp.fpfh(t["knn"], t["cloud"])
    assert torch.equal(again, t["fpfh"])


# ---------------------------------------------------------------------------------------------------------------- 3. match
def test_match_identity_rows_against_asymmetric_b(sp):
    """A = 33 unit rows, B small integers without symmetry: a . b picks one entry of b, every value is exact in float32, so a
    fragment layout that swaps rows with columns or misplaces a k step gives another index or distance."""
    a = np.zeros((33, 36), np.float32)
    a[np.arange(33), np.arange(33)] = 1.0
    j, k = np.meshgrid(np.arange(40), np.arange(33), indexing="ij")
    b = np.zeros((40, 36), np.float32)
    b[:, :33] = (7 * j + 3 * k + (j * k) % 5) % 13
    idx, d2 = sp.match_features(dev(a), dev(b))
    D = model.distances(a, b)
    want = D.argmin(1)
    assert np.array_equal(idx.cpu().numpy(), want), (idx.cpu().numpy(), want)
    assert np.array_equal(d2.cpu().numpy().astype(np.float64), D[np.arange(33), want])
    # and the other way round: 40 rows against the 33 unit rows
    idx, d2 = sp.match_features(dev(b), dev(a))
    assert np.array_equal(idx.cpu().numpy(), D.argmin(0))
    assert np.array_equal(d2.cpu().numpy().astype(np.float64), D.min(0))


def descriptors(n, seed):
    rs = np.random.RandomState(seed)
    g = rs.gamma(0.6, 1.0, (n, 3, 11)) + 1e-3
    g = 100.0 * g / g.sum(2, keepdims=True)
    out = np.zeros((n, 36), np.float32)
    out[:, :33] = g.reshape(n, 33)
    return out


def check_match(a, b, idx, d2, tag):
    D = model.distances(a, b)
    na2, nb2 = (a[:, :33].astype(np.float64) ** 2).sum(1), (b[:, :33].astype(np.float64) ** 2).sum(1)
    i = np.arange(len(a))
    assert ((idx >= 0) & (idx < len(b))).all()
    bound = 40 * U * (na2 + nb2[idx])
    over = D[i, idx] - D.min(1)
    derr = np.abs(d2.astype(np.float64) - D[i, idx])
    print(f"\n[match {tag}] {len(a)} x {len(b)}: index excess / bound <= {(over / bound).max():.3f}, |d2 - f64| / bound <= "
          f"{(derr / bound).max():.3f}, {int((idx != D.argmin(1)).sum())} indices differ from the float64 argmin", end="")
    assert (over <= 2 * bound).all()
    assert (derr <= bound).all()


@pytest.mark.parametrize("na", [1, 33])
@pytest.mark.parametrize("nb", [1, 31, 32, 33, 65])
def test_match_small_shapes(sp, na, nb):
    a, b = descriptors(na, 100 + na), descriptors(nb, 200 + nb)
    idx, d2 = sp.match_features(dev(a), dev(b))
    check_match(a, b, idx.cpu().numpy(), d2.cpu().numpy(), f"{na}x{nb}")


def test_match_empty_and_duplicates(sp):
    a = descriptors(70, 1)
    idx, d2 = sp.match_features(dev(a), dev(np.zeros((0, 36), np.float32)))
    assert (idx.cpu().numpy() == -1).all() and (d2.cpu().numpy() == np.float32(FLT_MAX)).all()
    assert sp.match_features(dev(np.zeros((0, 36), np.float32)), dev(a))[0].numel() == 0
    b = descriptors(300, 2)
    b[257], b[140], b[31] = b[5], b[5], b[5]          # the same row in four tiles and two stages
    b[290], b[64] = b[100], b[100]
    q = np.concatenate([b[5:6], b[100:101], a])
    idx, d2 = sp.match_features(dev(q), dev(b))
    idx = idx.cpu().numpy()
    assert idx[0] == 5 and idx[1] == 64 and d2[0].item() == 0.0 and d2[1].item() == 0.0
    check_match(q, b, idx, d2.cpu().numpy(), "duplicates")
    again, _ = sp.match_features(dev(q), dev(b))
    assert np.array_equal(again.cpu().numpy(), idx)


def test_match_and_mutual_on_the_bundled_pair(sp, bundled):
    fs, ft = bundled["source"]["fpfh"], bundled["target"]["fpfh"]
    a, b = fs.cpu().numpy(), ft.cpu().numpy()
    idx, d2 = sp.match_features(fs, ft)
    check_match(a, b, idx.cpu().numpy(), d2.cpu().numpy(), "bundled s->t")
    back, d2b = sp.match_features(ft, fs)
    check_match(b, a, back.cpu().numpy(), d2b.cpu().numpy(), "bundled t->s")
    corr = sp.match_features_mutual(fs, ft).cpu().numpy()
    # the model's pairs, and the rows whose decision (either direction) lies inside the bound
    D = model.distances(a, b)
    na2, nb2 = (a[:, :33].astype(np.float64) ** 2).sum(1), (b[:, :33].astype(np.float64) ** 2).sum(1)
    bound = 40 * U * (na2[:, None] + nb2[None, :])

    def candidates(D, bound, others):
        """per row: the entries whose float64 distance lies within the two bounds of the minimum (each computed distance is within
        its bound of the true one, so only these can win), and whether the decision among them is open: more than one, and not
        all the same row bit for bit (identical rows get identical computed distances; the tie goes to the lowest index on both
        sides)"""
        j = D.argmin(1)
        r = np.arange(len(D))
        cand = D - D[r, j][:, None] <= bound + bound[r, j][:, None]
        same = np.array([len(np.unique(others[c], axis=0)) == 1 for c in cand])
        return cand, (cand.sum(1) > 1) & ~same

    _, open_s = candidates(D, bound, b)
    cand_t, open_t = candidates(D.T, bound.T, a)
    s2t = D.argmin(1)
    i = np.arange(len(a))
    # row i's pair is open when its own match is, or when i is one of several rows that can win its match's way back (a way back
    # that is open among OTHER rows says "not i" on both sides)
    unsure = open_s | (open_t[s2t] & cand_t[s2t, i])
    want = model.mutual(a, b)
    got_of, want_of = np.full(len(a), -1), np.full(len(a), -1)
    got_of[corr[:, 0]], want_of[want[:, 0]] = corr[:, 1], want[:, 1]
    differ = got_of != want_of
    print(f"\n[mutual] {len(corr)} pairs on the device, {len(want)} in the model, {int(differ.sum())} rows differ, "
          f"{int(unsure.sum())} of {len(a)} rows have a decision inside the bound")
    assert (np.diff(corr[:, 0]) > 0).all() and len(np.unique(corr[:, 1])) == len(corr)
    assert not (differ & ~unsure).any()          # equal wherever no decision lies inside the bound
    assert differ.sum() <= 0.02 * len(a)         # at most 2 % of the rows excused
    assert np.array_equal(sp.match_features_mutual(fs, ft).cpu().numpy(), corr)


# --------------------------------------------------------------------------------------------------------------- 4. scores
def matches(m, seed):
    rs = np.random.RandomState(seed)
    cs = np.ones((m, 4), np.float32)
    cs[:, :3] = rs.uniform(-30, 30, (m, 3))
    T = model.rot_z(40.0)
    T[:3, 3] = [2.0, -1.0, 0.5]
    ct = np.ones((m, 4), np.float32)
    ct[:, :3] = cs[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3] + rs.normal(0, 0.15, (m, 3))
    wrong = rs.uniform(size=m) < 0.3
    wrong[:3] = False
    ct[wrong, :3] = rs.uniform(-30, 30, (int(wrong.sum()), 3))
    return cs, ct


@pytest.mark.parametrize("m", [3, 64, 465])
@pytest.mark.parametrize("hyps", [1, 64, 4096])
def test_scores(sp, m, hyps):
    cs, ct = matches(m, m)
    tau, min_edge, ratio, seed = 0.5, 1.0, 0.9, 1000 + m
    got = sp.ransac_scores(dev(cs), dev(ct), hyps, tau, min_edge, ratio, seed).cpu().numpy().astype(np.int64)
    want, parts = model.scores(cs, ct, hyps, seed, tau, min_edge, ratio)
    E = float(np.abs(np.concatenate([cs[:, :3], ct[:, :3]])).max()) + tau
    delta = 64 * U * E / 0.2
    with np.errstate(invalid="ignore"):
        slack = (np.abs(np.sqrt(parts["r2"]) - tau) <= delta).sum(1)
    excused = parts["near"]
    diff = np.abs(got - want)
    print(f"\n[scores] M {m} H {hyps}: {int(parts['valid'].sum())} pass the gates, best {int(want.max())}, {int(excused.sum())} excused, "
          f"{int((diff > 0).sum())} differ, delta {delta:.2e}, matches within delta of tau: {int(slack.sum())}")
    assert excused.sum() <= max(0.01 * hyps, 0)
    assert (diff <= slack)[~excused].all()
    if m >= 64 and hyps >= 64:
        assert parts["valid"].sum() >= 3 and want.max() > 0.4 * m  # the check is not vacuous


def test_scores_need_three_matches(sp):
    for m in (0, 1, 2):
        cs, ct = matches(max(m, 1), 5)
        got = sp.ransac_scores(dev(cs[:m]), dev(ct[:m]), 300, 1.0, 0.0, 0.9, 3)
        assert got.shape[0] == 300 and not got.any()


# ----------------------------------------------------------------------------------------------------------- 5. end to end
def registration(sp):
    return sp.Registration(sp.RegistrationParams(reg_type="GICP", max_correspondence_distance=2.0, max_iterations=30))


def test_end_to_end_bundled_pair(sp, bundled):
    S, Tg = bundled["source"], bundled["target"]
    T_true = bundled["T_true"]
    start = registration(sp).align(S["cloud"], Tg["cloud"], Tg["tree"])
    st, sr = model.pose_errors(start.T, T_true)
    print(f"\n[global registration] {S['cloud'].size()} / {Tg['cloud'].size()} points; align from the identity ends {st:.2f} m, "
          f"{sr:.3f} rad from the truth", end="")
    assert sr > 1.0  # the need
    prep = sp.PreparedTarget(sp.GridKNN.build(Tg["cloud"].points), Tg["cloud"].covs)
    ref = registration(sp).align_batch(S["cloud"], prep, [T_true.astype(np.float32)])[0]
    rt, rr = model.pose_errors(ref.T, T_true)
    gp = sp.GlobalRegistrationParams(hypotheses=50000, guesses=64, inlier_distance=1.0, min_edge=0.0, edge_ratio=0.9, seed=2024)
    reg = registration(sp)
    res, results, guesses = reg.align_global(S["cloud"], S["fpfh"], Tg["cloud"], Tg["fpfh"], prep, gp, return_all=True)
    gt, gr = model.pose_errors(res.T, T_true)
    near = sum(1 for T in guesses if model.pose_errors(T, T_true)[1] <= 0.1 and model.pose_errors(T, T_true)[0] <= 1.0)
    print(f" | align_batch from the truth {rt:.3e} m {rr:.3e} rad ({ref.inlier} inliers) | align_global {gt:.3e} m {gr:.3e} rad "
          f"({res.inlier} inliers, {getattr(res, 'matches', 0)} matches, {len(guesses)} guesses, {near} within 0.1 rad / 1 m of the truth)")
    assert res.converged and len(results) == len(guesses) == 64
    assert gt <= 2.0 * rt and gr <= 2.0 * rr, ((gt, gr), (rt, rr))
    # two runs: the same bytes
    res2, results2, guesses2 = registration(sp).align_global(S["cloud"], S["fpfh"], Tg["cloud"], Tg["fpfh"], prep, gp, return_all=True)
    assert res2.T.tobytes() == res.T.tobytes() and res2.hypothesis == res.hypothesis
    assert all(np.array_equal(a, b) for a, b in zip(guesses, guesses2))
    assert all(a.T.tobytes() == b.T.tobytes() and a.inlier == b.inlier and a.error == b.error for a, b in zip(results, results2))


def test_nothing_to_match_returns_unconverged(sp, bundled):
    S, Tg = bundled["source"], bundled["target"]
    prep = sp.PreparedTarget(sp.GridKNN.build(Tg["cloud"].points), Tg["cloud"].covs)
    gp = sp.GlobalRegistrationParams(hypotheses=1000, guesses=8)
    empty = sp.PointCloudShared(torch.empty((0, 4), dtype=torch.float32, device="cuda"))
    res = registration(sp).align_global(empty, torch.empty((0, 36), dtype=torch.float32, device="cuda"), Tg["cloud"], Tg["fpfh"], prep, gp)
    assert not res.converged and np.array_equal(res.T, np.eye(4, dtype=np.float32))
    # a single plane: every point has the same descriptor, one mutual pair survives
    flat_s = S["fpfh"][:1].repeat(S["cloud"].size(), 1).contiguous()
    flat_t = S["fpfh"][:1].repeat(Tg["cloud"].size(), 1).contiguous()
    assert sp.match_features_mutual(flat_s, flat_t).shape[0] == 1
    res, results, guesses = registration(sp).align_global(S["cloud"], flat_s, Tg["cloud"], flat_t, prep, gp, return_all=True)
    assert not res.converged and np.array_equal(res.T, np.eye(4, dtype=np.float32)) and not results and not guesses


# ------------------------------------------------------------------------------------------------------- the C++ facade
def fnv1a64(raw):
    h = 1469598103934665603
    for byte in raw:
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_facade(sp, bundled, tmp_path):
    """feature::compute_fpfh, registration::global_guesses and Registration::align_global of the C++ facade (tests/cpp/
    test_global_registration.cpp, built here with the facade tests' flags) on the prepared bundled pair: the descriptor bytes, the 64
    guesses and the winner are the Python mirror's, bit for bit."""
    import subprocess

    from test_gpu_lidar_odometry import build

    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = build(os.path.join(cpp, "test_global_registration.cpp"), os.path.join(cpp, "test_global_registration"))
    S, Tg = bundled["source"], bundled["target"]
    path = str(tmp_path / "pair.bin")
    with open(path, "wb") as f:
        f.write(np.array([S["cloud"].size(), Tg["cloud"].size(), 20], np.int32).tobytes())
        for c in (S, Tg):
            for t in (c["cloud"].points, c["cloud"].normals, c["cloud"].covs):
                f.write(np.ascontiguousarray(t.cpu().numpy(), np.float32).tobytes())
            f.write(np.ascontiguousarray(c["idx"], np.int32).tobytes())
            f.write(np.ascontiguousarray(c["d2"], np.float32).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout[-4000:]
    for name in ("descriptors", "guesses", "align_global", "nothing_to_match"):
        assert f"[  OK  ] {name}" in r.stdout, name
    poses, sums, scalars = {}, {}, None
    for line in r.stdout.splitlines():
        if line.startswith("T "):
            name, *words = line[2:].split()
            poses[name] = np.array([int(x, 16) for x in words], np.uint32).view(np.float32).reshape(4, 4).T
        elif line.startswith("F "):
            sums[line.split()[1]] = int(line.split()[2], 16)
        elif line.startswith("R winner"):
            scalars = line.split()[2:]
    assert sums["source"] == fnv1a64(S["fpfh"].cpu().numpy().tobytes()) and sums["target"] == fnv1a64(Tg["fpfh"].cpu().numpy().tobytes())
    prep = sp.PreparedTarget(sp.GridKNN.build(Tg["cloud"].points, points_per_cell=0.5), Tg["cloud"].covs)  # the facade's grid
    gp = sp.GlobalRegistrationParams(hypotheses=50000, guesses=64, inlier_distance=1.0, min_edge=0.0, edge_ratio=0.9, seed=2024)
    # (the facade leaves a source of up to 4096 points in its order: the order decides how the sums are grouped)
    res, _, guesses = registration(sp).align_global(S["cloud"], S["fpfh"], Tg["cloud"], Tg["fpfh"], prep, gp, return_all=True,
                                                    sort_by_cell="presorted")
    assert len(guesses) == 64
    for i, T in enumerate(guesses):
        assert poses[f"guess{i}"].tobytes() == np.ascontiguousarray(T, np.float32).tobytes(), i
    assert poses["winner"].tobytes() == res.T.tobytes()
    assert (int(scalars[0]), int(scalars[1]), int(scalars[2])) == (res.iterations, int(res.converged), res.inlier)
    assert int(scalars[3], 16) == int(np.float32(res.error).view(np.uint32))
