"""The prepared source in wave tiles (csrc/registration_device.h, FusedParams): 64 consecutive prepared points are one block
of 9 x 64 floats, sub-plane k (x y z | xx xy xz yy yz zz) at word 64 k, the point's lane at word i % 64 — one address per point,
nine loads at fixed offsets from it.

  * layout: every prepared point's nine words sit where the formula says and are the plane-regularised values of
    covariance.update_covariance_plane, exactly, through the presorted path and the path that sorts by cell; a buffer full of NaN
    before the preparation (the unused lanes of the last tile, and for POINT_TO_DISTRIBUTION the covariance sub-planes, stay NaN)
    never reaches a result;
  * bits: a 6-iteration alignment is bit-identical with the correspondence reuse on and off and lands on the generic loop's
    pose, for GICP, POINT_TO_DISTRIBUTION, a robust loss and a source of which a third lies outside the overlap (the early
    return in front of the loads that follow the search);
  * the device-resident optimiser (LM + Geman-McClure) reads the same tiles and lands on the per-step loop's pose.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NS = [1, 63, 64, 65, 1000, 1025]
TILE, PLANES = 64, 9
N_TARGET = 3000


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def random_spd_covs(n, seed):
    """n covariances in the stored layout (16 floats: a 4x4 whose 3x3 block counts), B B^T + 1e-4 I with B ~ N(0, 0.05^2)"""
    B = np.random.RandomState(seed).normal(0.0, 0.05, size=(n, 3, 3))
    C3 = B @ B.transpose(0, 2, 1) + 1e-4 * np.eye(3)
    out = np.zeros((n, 4, 4), np.float32)
    out[:, :3, :3] = C3.astype(np.float32)
    out[:, :3, :3] = 0.5 * (out[:, :3, :3] + out[:, :3, :3].transpose(0, 2, 1))  # symmetric in float32 too
    return out.reshape(n, 16)


@pytest.fixture(scope="module")
def scene(sp):
    """A small target with a known pose (config 4's density and twist), its covariances from 20 neighbours; the source points
    are the first n of its counterpart cloud, with random SPD covariances."""
    from sycl_points_amd.synthetic import gicp_pair

    src, tgt, T_gt = gicp_pair(N_TARGET, 10.0 * (N_TARGET / 1e6) ** (1.0 / 3.0), seed=2718)
    Tg = sp.PointCloudShared(dev(tgt))
    Tg.covs = sp.GridKNN.build(Tg.points, points_per_cell=6.0).self_knn(20, want_knn=False, want_covs=True)[1]
    grid = sp.GridKNN.build(Tg.points)
    preps = {r: sp.PreparedTarget(grid, Tg.covs, reg_type=r) for r in ("GICP", "POINT_TO_DISTRIBUTION")}
    scov = random_spd_covs(N_TARGET, 5)
    return src, scov, Tg, grid, preps, T_gt


def tile_word(i, k):
    """the documented formula: float index of sub-plane k of prepared point i"""
    return (i // TILE) * (PLANES * TILE) + k * TILE + (i % TILE)


def read_tiles(sp, psrc):
    L = sp._lib.lib()
    nf = L.sp_internal_source_tile_floats(psrc._h)
    buf = torch.empty(nf, dtype=torch.float32, device="cuda")
    sp.check(L.sp_internal_source_tiles_copy(psrc._h, sp._ptr(buf), nf, 0, sp._stream()))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def fill_tiles_nan(sp, psrc):
    L = sp._lib.lib()
    nf = L.sp_internal_source_tile_floats(psrc._h)
    buf = torch.full((nf,), float("nan"), dtype=torch.float32, device="cuda")
    sp.check(L.sp_internal_source_tiles_copy(psrc._h, sp._ptr(buf), nf, 1, sp._stream()))
    torch.cuda.synchronize()
    return nf


def expected_words(sp, pts, covs):
    """(n, 9): the point and the upper triangle of its plane-regularised covariance as prepare_source_kernel symmetrises it,
    from the library's own update_covariance_plane — float32 sums and halvings, exact on both sides"""
    P = sp.covariance.update_covariance_plane(dev(covs)).cpu().numpy().reshape(-1, 4, 4)
    half = np.float32(0.5)
    sym = lambda a, b: (P[:, a, b] + P[:, b, a]) * half  # noqa: E731
    return np.stack([pts[:, 0], pts[:, 1], pts[:, 2], P[:, 0, 0], sym(0, 1), sym(0, 2), P[:, 1, 1], sym(1, 2), P[:, 2, 2]],
                    axis=1).astype(np.float32)


@pytest.mark.parametrize("reg_type", ["GICP", "POINT_TO_DISTRIBUTION"])
@pytest.mark.parametrize("mode", ["presorted", True], ids=["presorted", "sort-by-cell"])
@pytest.mark.parametrize("n", NS)
def test_layout_of_the_prepared_source(sp, scene, n, mode, reg_type):
    src, scov, Tg, grid, preps, T_gt = scene
    pts, covs = src[:n], scov[:n]
    S = sp.PointCloudShared(dev(pts), covs=dev(covs))
    p = sp.RegistrationParams(reg_type=reg_type, criteria_translation=0.0, criteria_rotation=0.0, max_iterations=6)
    reg = sp.Registration(p)
    psrc, _ = reg._prepared_source(n)
    nf = fill_tiles_nan(sp, psrc)
    assert nf == (n + TILE - 1) // TILE * PLANES * TILE  # whole tiles, n need not be a multiple of 64
    T_dev, lin, delta = reg.align_fused_loop(S, preps[reg_type], sort_by_cell=mode)
    torch.cuda.synchronize()
    # no unused lane (NaN) influenced a result
    assert np.isfinite(T_dev.cpu().numpy()).all() and np.isfinite(lin.cpu().numpy()[:44]).all()
    assert np.isfinite(delta.cpu().numpy()).all()
    tiles = read_tiles(sp, psrc)
    used = PLANES if reg_type == "GICP" else 3  # POINT_TO_DISTRIBUTION never reads, and never writes, a source covariance
    idx = np.arange(n)
    got = np.stack([tiles[tile_word(idx, k)] for k in range(PLANES)], axis=1)
    want = expected_words(sp, pts, covs)
    if mode == "presorted":
        order = idx
    else:  # the prepared order is a permutation of the source: find it by the (distinct) points
        key = lambda a: [tuple(r) for r in a[:, :3].view(np.uint32)]  # noqa: E731
        where = {k: i for i, k in enumerate(key(want))}
        assert len(where) == n
        order = np.array([where[k] for k in key(got)])
        assert np.array_equal(np.sort(order), idx)
    assert np.array_equal(got[:, :used].view(np.uint32), want[order][:, :used].view(np.uint32))
    # what the preparation does not write stays as it was: the lanes past n of the last tile, the unused sub-planes
    written = np.zeros(nf, bool)
    for k in range(used):
        written[tile_word(idx, k)] = True
    assert np.isnan(tiles[~written]).all() and not np.isnan(tiles[written]).any()


def align_fused(sp, S, prep, p, reuse, mode, T0=None):
    reg = sp.Registration(p)
    reg._set_source_option("reuse", reuse)
    T_dev, lin, delta = reg.align_fused_loop(S, prep, initial_guess=T0, sort_by_cell=mode)
    torch.cuda.synchronize()
    return T_dev.cpu().numpy().copy(), lin.cpu().numpy().copy(), delta.cpu().numpy().copy()


PARITY_CASES = [
    dict(reg_type="GICP", loss="NONE", scale=10.0),
    dict(reg_type="POINT_TO_DISTRIBUTION", loss="NONE", scale=10.0),
    dict(reg_type="GICP", loss="CAUCHY", scale=0.3),
    dict(reg_type="GICP", loss="NONE", scale=10.0, outside=True),  # a third of the source outside the overlap
]


@pytest.mark.parametrize("case", PARITY_CASES, ids=lambda c: f"{c['reg_type']}-{c['loss']}" + ("-third-outside" if c.get("outside") else ""))
@pytest.mark.parametrize("n", NS)
def test_reuse_on_off_bit_identical_and_generic_parity(sp, scene, n, case):
    src, scov, Tg, grid, preps, T_gt = scene
    pts, covs = src[:n].copy(), scov[:n]
    max_corr = 2.0
    if case.get("outside"):  # no target within any useful distance of these: searched, nothing found, the early return
        pts[::3, :3] += np.float32([37.0, -21.0, 9.0])
        max_corr = 0.5
    S = sp.PointCloudShared(dev(pts), covs=dev(covs))
    p = sp.RegistrationParams(reg_type=case["reg_type"], robust_type=case["loss"], robust_default_scale=case["scale"],
                              criteria_translation=0.0, criteria_rotation=0.0, max_iterations=6,
                              max_correspondence_distance=max_corr)
    prep = preps[case["reg_type"]]
    on, off = align_fused(sp, S, prep, p, 2, "presorted"), align_fused(sp, S, prep, p, 0, "presorted")
    for a, b in zip(on, off):  # pose, linear system, last update: reuse on == reuse off, bit for bit
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    lin = sp.Registration._read_lin(torch.from_numpy(on[1]))
    assert lin.inlier == (n - len(pts[::3]) if case.get("outside") else n)
    # the generic loop (KNNBase search + K11 + device solve) lands on the same pose: the tolerance of the existing parity test
    # of this pair (test_gpu_benchmarked_path.py)
    regg = sp.Registration(p)
    Tgen, _, _ = regg.align_device_loop(S, Tg, grid, iterations=6)
    T = on[0].reshape(4, 4).T
    diff = np.abs(regg.T_from_device(Tgen) - T).max()
    print(f"n={n} {case}: |T_fused - T_generic| = {diff:.3e}, |T_fused - T_gt| = {np.abs(T - T_gt).max():.3e}")
    assert diff < 2e-6


def test_optimiser_reads_the_same_tiles(sp, scene):
    """LM + Geman-McClure (BASELINE config 1's optimiser and kernel) on 1000 points: the device-resident launch against the
    per-step loop of the same library, the tolerance of test_gpu_optimize.py for this pair."""
    src, scov, Tg, grid, preps, T_gt = scene
    n = 1000
    S = sp.PointCloudShared(dev(src[:n]), covs=dev(scov[:n]))
    p = sp.RegistrationParams(robust_type="GEMAN_MCCLURE", robust_default_scale=0.5, optimization_method="LM", max_iterations=25)
    T0 = np.eye(4, dtype=np.float32)
    T0[:3, 3] = [0.05, -0.04, 0.03]
    res = sp.Registration(p).align_optimize(S, preps["GICP"], T0, [0.5])
    assert res is not None, "the persistent launch must be available on an idle MI355X"
    host = sp.Registration(p).align_prepared(S, preps["GICP"], initial_guess=T0, device_resident=False)
    print(f"|T_launch - T_steps| = {np.abs(host.T - res.T).max():.3e}, |T - T_gt| = {np.abs(res.T - T_gt).max():.3e}")
    assert np.abs(host.T - res.T).max() < 2e-6 and host.iterations == res.iterations and host.converged == res.converged
    assert host.inlier == res.inlier
    assert np.abs(res.T - T_gt).max() < 5e-3  # (random source covariances, 1000 noisy points: the known pose to the noise's size)
