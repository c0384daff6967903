"""The prepared linearisation against what the PARENT build of this change computed, byte for byte.

How the per-point algebra is compiled (csrc/sp_linearize.h; no SLP vectorisation in its two translation units) must not move a
bit of any sum. tests/golden/linearize_pairs_parent.npz holds, recorded on the parent commit's library by
profiles/record_linearize_pairs.py (which runs the functions of THIS file), for the five losses x {GICP, POINT_TO_DISTRIBUTION}
at n = 1, 63, 64, 65 (lane and tile edges), 1025 (workgroup edge) and 5000 (every twentieth source point moved outside
max_correspondence_distance, so cache rows with index -1 occur):

  * the 128-byte fan-in row (28 sums, the inlier count as two floats, the searched count) of ONE sp_gicp_align_step at a fixed
    pose whose rotation has nine distinct non-zero entries;
  * pose, linear system and last update of a 5-iteration sp_gicp_align_fused from that pose.

Both are asserted equal as bytes on this build, with the correspondence reuse as shipped and with reuse = 0, where every launch
searches every point. The inputs are regenerated here; their checksums are in the file, so that an input that differs (another
numpy, another device) is reported as that and not as a wrong sum.
"""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "linearize_pairs_parent.npz")
NS = [1, 63, 64, 65, 1025, 5000]
LOSSES = ["NONE", "HUBER", "TUKEY", "CAUCHY", "GEMAN_MCCLURE"]
REGS = ["GICP", "POINT_TO_DISTRIBUTION"]
N_TARGET = 6000
MAX_CORR = 0.5
ROBUST_SCALE = 0.3
ITERATIONS = 5
# rotation vector and translation of the fixed pose (the pose itself, float32, is kept in the golden file)
POSE_ROTVEC, POSE_TRANS = (0.021, -0.017, 0.033), (0.05, -0.04, 0.03)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def fixed_pose():
    w = np.array(POSE_ROTVEC, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = POSE_TRANS
    return T.astype(np.float32)


def random_spd_covs(n, seed):
    """n covariances in the stored layout (16 floats: a 4x4 whose 3x3 block counts), B B^T + 1e-4 I with B ~ N(0, 0.05^2)"""
    B = np.random.RandomState(seed).normal(0.0, 0.05, size=(n, 3, 3))
    C3 = B @ B.transpose(0, 2, 1) + 1e-4 * np.eye(3)
    out = np.zeros((n, 4, 4), np.float32)
    out[:, :3, :3] = C3.astype(np.float32)
    out[:, :3, :3] = 0.5 * (out[:, :3, :3] + out[:, :3, :3].transpose(0, 2, 1))
    return out.reshape(n, 16)


def make_scene(sp):
    """Target with its covariances from 20 neighbours and both prepared forms; the source cloud of its pair with random SPD
    covariances. Returns the scene and the checksums of every input."""
    from sycl_points_amd.synthetic import gicp_pair

    src, tgt, _ = gicp_pair(N_TARGET, 10.0 * (N_TARGET / 1e6) ** (1.0 / 3.0), seed=1618)
    Tg = sp.PointCloudShared(dev(tgt))
    Tg.covs = sp.GridKNN.build(Tg.points, points_per_cell=6.0).self_knn(20, want_knn=False, want_covs=True)[1]
    grid = sp.GridKNN.build(Tg.points)
    preps = {r: sp.PreparedTarget(grid, Tg.covs, reg_type=r) for r in REGS}
    scov = random_spd_covs(N_TARGET, 7)
    torch.cuda.synchronize()
    sums = np.array([crc(src), crc(tgt), crc(scov), crc(Tg.covs.cpu().numpy())], np.uint32)
    return dict(src=src, scov=scov, Tg=Tg, grid=grid, preps=preps, keep=(Tg, grid)), sums


def source_cloud(sp, scene, n):
    pts, covs = scene["src"][:n].copy(), scene["scov"][:n]
    if n == 5000:  # every twentieth point: no target within max_correspondence_distance, whatever the pose
        pts[::20, :3] += np.float32([37.0, -21.0, 9.0])
    return sp.PointCloudShared(dev(pts), covs=dev(covs))


def params(sp, reg_type, loss):
    return sp.RegistrationParams(reg_type=reg_type, robust_type=loss, robust_default_scale=ROBUST_SCALE if loss != "NONE" else 10.0,
                                 criteria_translation=0.0, criteria_rotation=0.0, max_iterations=ITERATIONS,
                                 max_correspondence_distance=MAX_CORR)


def step_row(sp, S, prep, p, T0, reuse):
    """The fan-in row of launch 0 of an alignment at T0: one sp_gicp_align_step(k = 0, rows_all_reduced = 2)."""
    L = sp._lib.lib()
    reg = sp.Registration(p)
    if reuse is not None:
        reg._set_source_option("reuse", reuse)
    device = S.points.device
    ws, lin = reg._buffers(device)
    n = S.size()
    T_dev = torch.from_numpy(sp._T16(T0).reshape(-1).copy()).to(device)
    reg._prepared_source(n)
    reg._psrc.prepare(prep, S, T_dev, "presorted")
    fp = reg._factor_params(p.robust_default_scale)
    gn = sp.GnParams(p.gn_lambda, p.criteria_rotation, p.criteria_translation)
    sp.check(L.sp_gicp_align_step(prep._h, reg._psrc._h, sp._ptr(T_dev), C.byref(fp), C.byref(gn), 0, 2, None, None, sp._ptr(lin),
                                  sp._ptr(ws), ws.numel(), sp._stream()))
    nf = C.c_size_t(0)
    off = (L.sp_gicp_align_row(sp._ptr(ws), 0, C.byref(nf)) - ws.data_ptr()) // 4
    torch.cuda.synchronize()
    return ws.view(torch.float32)[off:off + nf.value].cpu().numpy().copy()


def aligned(sp, S, prep, p, T0, reuse):
    """Pose (16), linear system and last update after ITERATIONS iterations of sp_gicp_align_fused from T0."""
    reg = sp.Registration(p)
    if reuse is not None:
        reg._set_source_option("reuse", reuse)
    T_dev, lin, delta = reg.align_fused_loop(S, prep, initial_guess=T0, sort_by_cell="presorted")
    torch.cuda.synchronize()
    return (T_dev.cpu().numpy().copy(), lin.cpu().numpy().reshape(-1).view(np.float32)[:46].copy(), delta.cpu().numpy().copy())


def case_index(reg_type, loss, n):
    """row of the golden file's arrays `row`, `T`, `lin`, `delta` that holds this case"""
    return (REGS.index(reg_type) * len(LOSSES) + LOSSES.index(loss)) * len(NS) + NS.index(n)


def compute_case(sp, scene, reg_type, loss, n, T0, reuse):
    S = source_cloud(sp, scene, n)
    p = params(sp, reg_type, loss)
    prep = scene["preps"][reg_type]
    T, lin, delta = aligned(sp, S, prep, p, T0, reuse)
    return dict(row=step_row(sp, S, prep, p, T0, reuse), T=T, lin=lin, delta=delta)


# ------------------------------------------------------------------------------------------------------------ the test
@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def scene(sp, golden):
    sc, sums = make_scene(sp)
    assert np.array_equal(sums, golden["input_crc32"]), "the regenerated inputs differ from the recorded ones (src, tgt, scov, tcov)"
    assert np.array_equal(fixed_pose().view(np.uint32), golden["T0"].view(np.uint32)), "the fixed pose differs from the recorded one"
    return sc


def test_golden_is_the_parents(golden):
    assert len(str(golden["parent_commit"])) == 40
    assert sorted(golden["ns"].tolist()) == NS and len(golden["row"]) == len(REGS) * len(LOSSES) * len(NS)
    R = golden["T0"][:3, :3].reshape(-1)
    assert (R != 0).all() and len(set(R.tolist())) == 9  # nine distinct non-zero entries: a swapped pair of them shows


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("reg_type", REGS)
def test_sums_and_pose_are_the_parents_bytes(sp, scene, golden, reg_type, loss, n):
    T0 = golden["T0"]
    for reuse in (None, 0):  # as shipped; every launch searches every point
        got = compute_case(sp, scene, reg_type, loss, n, T0, reuse)
        for what, v in got.items():
            want = golden[what][case_index(reg_type, loss, n)]
            assert v.dtype == np.float32 and v.shape == want.shape
            assert np.array_equal(v.view(np.uint32), want.view(np.uint32)), \
                f"{what} differs from the parent's (reuse={reuse}): {v} != {want}"
    row = golden["row"][case_index(reg_type, loss, n)]
    inliers = int(row[29]) * 4096 + int(row[28])  # (the count travels as two exactly-summable floats)
    moved = len(range(0, n, 20)) if n == 5000 else 0
    assert 0.9 * (n - moved) - 1 <= inliers <= n - moved  # the moved points have no correspondence; nearly all others have one
