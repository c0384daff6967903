"""Every device entry that forms a covariance or a normal, on the families of tests/f64_features.py, per row:

  * against the float64 model: error <= 4 K eps32 kappa_row, K the oracle's measured constant (f64_features.ORACLE_K; the factor 4
    covers the device's own acosf / cosf / cbrtf, a few ulp from the host's and amplified like every other rounding). No row is
    left out and no percentile is taken; the degenerate families assert their invariants;
  * against the CPU oracle: the same bits for K5, the plain and the M-estimated covariance and inverse(); everything that goes
    through the eigen-solver within 4 (2 K) eps32 kappa_row (device and oracle may each be K-ish out, in opposite directions);
  * a second launch gives the same bits.

The entries: sp_internal_eigen3 / sp_internal_inverse3 (symmetric_eigen3 and inverse on their own), covariance.estimate,
estimate_normals, extract_normals, update_covariance_plane, normalize_covariance, estimate_robust, and the grid's fused self-kNN with
covariances and normals in every kernel mode. sp_cov_estimate is also run at the shapes that reach both of its kernels and every
tail of the LDS staging, sp_cov_estimate_robust at both median parities and its identity / zero-inverse branches.

`pytest -s` prints the measured worst error / (eps32 kappa) per quantity: the device columns of the table in DESIGN.md section 2.2."""
import ctypes as C

import numpy as np
import pytest

import f64_features as F

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


class DeviceFeatures:
    """The f64_features interface over the device entries."""

    def __init__(self, sp):
        from sycl_points_amd import _lib

        self.sp, self.L, self.check = sp, _lib.lib(), _lib.check
        self.stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def eigen3(self, rows):
        r = dev(rows)
        vals = torch.empty((len(rows), 3), dtype=torch.float32, device="cuda")
        vecs = torch.empty((len(rows), 16), dtype=torch.float32, device="cuda")
        self.check(self.L.sp_internal_eigen3(r.data_ptr(), len(rows), vals.data_ptr(), vecs.data_ptr(), self.stream()))
        return host(vals), F.cov3(host(vecs)).astype(np.float32)

    def inverse3(self, rows):
        r = dev(rows)
        out = torch.empty((len(rows), 16), dtype=torch.float32, device="cuda")
        self.check(self.L.sp_internal_inverse3(r.data_ptr(), len(rows), out.data_ptr(), self.stream()))
        return F.cov3(host(out)).astype(np.float32)

    def cov(self, pts, idx):
        return host(self.sp.covariance.estimate(dev(idx), dev(pts)))

    def normals_knn(self, pts, idx):
        return host(self.sp.covariance.estimate_normals(dev(idx), dev(pts)))

    def normals_cov(self, pts, covs):
        return host(self.sp.covariance.extract_normals(dev(pts), dev(covs)))

    def plane(self, rows):
        return host(self.sp.covariance.update_covariance_plane(dev(rows)))

    def normalize(self, rows):
        return host(self.sp.covariance.normalize_covariance(dev(rows)))

    def robust(self, pts, idx, loss, mad_scale, min_scale, iterations):
        return host(self.sp.covariance.estimate_robust(dev(idx), dev(pts), loss, mad_scale, min_scale, iterations))


@pytest.fixture(scope="module")
def device_out(sp):
    return F.collect(DeviceFeatures(sp))


@pytest.fixture(scope="module")
def oracle_out(orc):
    return F.cached("oracle_out", lambda: F.collect(F.OracleFeatures(orc)))


def quantity(key):
    return {"normals_knn": "normal", "normals_cov": "normal"}.get(key[0], key[0])


def report(tag, res):
    print(f"\n[gpu-features-f64] worst error / (eps32 * kappa), {tag}:")
    for q, (v, key) in sorted(F.worst(res).items()):
        print(f"[gpu-features-f64]   {q:12s} {v:9.3g}   (K = {F.ORACLE_K[q]:g}) at {key}")
    for key, v in sorted(res.items(), key=str):
        print(f"[gpu-features-f64]     {str(key):60s} {v:9.3g}")


def test_every_row_against_float64(device_out):
    res = F.score(device_out)   # asserts the invariants of every family on the way
    report("device against float64", res)
    for key, v in res.items():
        assert v <= 4.0 * F.ORACLE_K[quantity(key)], (key, v)


# the outputs that do not go through acosf / cosf / cbrtf: bit for bit the oracle's
BITWISE = ("cov", "robust", "inverse")


def test_every_row_against_the_oracle(device_out, oracle_out):
    for key, got in device_out.items():
        if key[0] in BITWISE:
            assert np.array_equal(got, oracle_out[key]), f"{key}: device and oracle differ in a bit"
    res = F.score(device_out, other=oracle_out)
    report("device against the oracle", res)
    for key, v in res.items():
        assert v <= 4.0 * 2.0 * F.ORACLE_K[quantity(key)], (key, v)


def test_a_second_launch_gives_the_same_bits(sp, device_out):
    again = F.collect(DeviceFeatures(sp))
    assert again.keys() == device_out.keys()
    for key, got in again.items():
        for a, b in zip(got if isinstance(got, tuple) else (got,), device_out[key] if isinstance(got, tuple) else (device_out[key],)):
            assert np.array_equal(a, b), key


def test_flip_rule(device_out, oracle_out):
    F.score_flip(device_out["normals_cov", "flip"], oracle_out["normals_cov", "flip"])


# ---------------------------------------------------------------------------------------------- sp_cov_estimate: every path
def shaped_lists(rs, n_rows, n_pts, k):
    """Neighbour lists with -1 at the front, in the middle and at the tail, rows with exactly 3 and exactly 4 valid entries."""
    idx = rs.randint(0, n_pts, (n_rows, k)).astype(np.int32)
    if k >= 2:
        idx[0::5, 0] = -1
        idx[1::5, k // 2] = -1
        idx[2::5, k - 1] = -1
    if k >= 5:
        for first, valid in ((3, 3), (4, 4)):
            rows = np.arange(first, n_rows, 10)
            idx[rows] = -1
            for r in rows:
                idx[r, rs.choice(k, valid, replace=False)] = rs.randint(0, n_pts, valid)
    return idx


@pytest.mark.parametrize("k", [1, 3, 4, 5, 7, 20, 63, 64, 65])
def test_cov_estimate_same_bits_on_every_path(sp, orc, k):
    """cov_kernel (lists staged through LDS: the 16-byte body and the word-by-word tail, 64 KB of dynamic LDS at k = 64) and
    cov_direct_kernel (k = 65, or a list array 4 bytes off 16-byte alignment) store the same bits, the oracle's. A missing direct
    path would answer k = 65 and the misaligned view with an error code, not with covariances."""
    rs = np.random.RandomState(1000 + k)
    for n in (1, 255, 256, 257, 4097):
        pts = np.ones((n, 4), np.float32)
        pts[:, :3] = rs.uniform(-3.0, 3.0, (n, 3))
        idx = shaped_lists(rs, n, n, k)
        want = orc.cov_estimate(pts, idx)
        P = dev(pts)
        aligned = dev(idx)
        assert aligned.data_ptr() % 16 == 0
        store = torch.full((n * k + 8,), -7, dtype=torch.int32, device="cuda")
        view = store[1:1 + n * k].view(n, k)
        view.copy_(aligned)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        a = host(sp.covariance.estimate(aligned, P))
        b = host(sp.covariance.estimate(view, P))
        assert np.array_equal(a, want), (n, k, "aligned lists")
        assert np.array_equal(b, want), (n, k, "lists 4 bytes off 16-byte alignment")
        assert np.array_equal(host(sp.covariance.estimate(aligned, P)), a), (n, k, "second launch")
        few = (idx >= 0).sum(axis=1) < 4
        eye = F.cov16(np.broadcast_to(np.eye(3, dtype=np.float32), (int(few.sum()), 3, 3)))
        assert np.array_equal(a[few], eye), (n, k, "fewer than 4 valid neighbours: identity")
        if k >= 5 and n >= 255:
            valid = (idx >= 0).sum(axis=1)
            assert (valid == 3).any() and (valid == 4).any() and not few.all()


# ---------------------------------------------------------------------------------------------- sp_cov_estimate_robust
@pytest.mark.parametrize("k", [4, 5, 63, 64])
def test_cov_estimate_robust_shapes(sp, orc, k):
    """Both parities of the median, -1 in the middle of a row, 0 / 1 / 5 rounds, every loss: the oracle's bits."""
    rs = np.random.RandomState(2000 + k)
    n = 300
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = rs.normal(size=(n, 3)) * np.array([1.0, 0.6, 0.3])
    idx = rs.randint(0, n, (n, k)).astype(np.int32)
    idx[::3, k // 2] = -1   # (k = 4: three valid neighbours are left, the identity; k = 5: four)
    if k > 5:
        idx[1::7, 0] = -1
    P, I = dev(pts), dev(idx)
    for loss in F.ROBUST_LOSSES:
        for it in (0, 1, 5):
            got = host(sp.covariance.estimate_robust(I, P, loss, 1.25, 0.5, it))
            assert np.isfinite(got).all()
            assert np.array_equal(got, orc.cov_estimate_robust(pts, idx, loss, 1.25, 0.5, it)), (k, loss, it)
            if it == 0:
                assert np.array_equal(got, host(sp.covariance.estimate(I, P)))


def test_cov_estimate_robust_identity_zero_inverse_and_limit(sp, orc):
    rs = np.random.RandomState(77)
    k, n = 20, 40
    nb = F.neighbourhoods(rs, (0.05, 0.3, 1.0), n // k, k)
    # a row whose TUKEY weights all vanish: 12 of its 20 slots are padding (distance 0), so the median is 0 and the scale the
    # floor, 1e-3, which every valid neighbour's distance exceeds: total weight 0 < FLT_EPSILON, the identity comes out of round 1
    idx = nb.idx.copy()
    idx[:, 4:16] = -1
    m = F.robust_covariance(nb.pts, idx, "TUKEY", 1.25, 1e-3, 1)
    assert np.array_equal(m, np.broadcast_to(np.eye(3), m.shape))   # the model agrees that this is the case built here
    got = host(sp.covariance.estimate_robust(dev(idx), dev(nb.pts), "TUKEY", 1.25, 1e-3, 1))
    assert np.array_equal(got, F.cov16(np.broadcast_to(np.eye(3, dtype=np.float32), (n, 3, 3))))
    assert np.array_equal(got, orc.cov_estimate_robust(nb.pts, idx, "TUKEY", 1.25, 1e-3, 1))
    # exactly coplanar neighbours: singular covariance, inverse() answers Zero, every weight stays 1: the plain covariance
    flat = nb.pts.copy()
    flat[:, 2] = 0.0
    plain = host(sp.covariance.estimate(dev(nb.idx), dev(flat)))
    assert np.abs(np.linalg.det(F.cov3(plain))).max() <= F.DET_BELOW
    for loss in F.ROBUST_LOSSES:
        got = host(sp.covariance.estimate_robust(dev(nb.idx), dev(flat), loss, 1.25, 0.5, 5))
        assert np.array_equal(got, plain), loss
        assert np.array_equal(got, orc.cov_estimate_robust(flat, nb.idx, loss, 1.25, 0.5, 5)), loss
    # k = 65: the reference's message
    wide = dev(np.zeros((n, 65), np.int32))
    with pytest.raises(sp.SpError, match=r"\[covariance::estimate_robust_async\] neighbor K is too large. MAX_K is 64"):
        sp.covariance.estimate_robust(wide, dev(nb.pts), "HUBER", 1.25, 0.5, 1)


# ---------------------------------------------------------------------------------------------- the grid's fused epilogues
@pytest.fixture(scope="module")
def degenerate_cloud():
    """Neighbourhoods that are the degenerate ones: a square-lattice plane z = const (lambda1 == lambda2), a line, duplicates."""
    side = 60
    gx, gy = np.meshgrid(np.arange(side, dtype=np.float32), np.arange(side, dtype=np.float32))
    plane = np.stack([gx.ravel() * 0.125, gy.ravel() * 0.125, np.full(side * side, 0.5, np.float32)], axis=1)
    line = np.float32([10.0, -2.0, 1.0]) + np.arange(1500, dtype=np.float32)[:, None] * np.float32([0.0625, 0.03125, -0.015625])
    rs = np.random.RandomState(5)
    dup = np.repeat(rs.uniform(-6.0, -3.0, (6, 3)).astype(np.float32), 20, axis=0)
    pts = np.ones((len(plane) + len(line) + len(dup), 4), np.float32)
    pts[:, :3] = np.concatenate([plane, line, dup])
    order = rs.permutation(len(pts))
    return pts[order], order < len(plane)


# the lane kernel (mode 0, k <= 7), the selection and its wave-per-query list (mode 0 above 7; mode 3 from 7), the wave-cooperative
# kernel (mode 2): the (k, mode) pairs tests/test_gpu_parity.py and tests/test_gpu_edge_cases.py switch between
@pytest.mark.parametrize("k, mode", [(4, 0), (7, 0), (8, 0), (20, 0), (3, 2), (10, 2), (7, 3), (20, 3)])
def test_grid_fused_epilogues_on_degenerate_neighbourhoods(sp, degenerate_cloud, k, mode):
    """A covariance or a normal made inside a self-kNN kernel carries the bits sp_cov_estimate / sp_normals_from_cov store for the
    same neighbour lists, where the neighbourhoods are degenerate (csrc/sp_cov_normal.h's promise, at its hardest inputs)."""
    pts, on_plane = degenerate_cloud
    P = dev(pts)
    for ppc in (1.0, 8.0):
        grid = sp.GridKNN.build(P, points_per_cell=ppc)
        grid._set_option("self_knn_mode", mode)
        res, covs, nrm = grid.self_knn(k, want_knn=True, want_covs=True, want_normals=True)
        assert bool(torch.isfinite(covs).all()) and bool(torch.isfinite(nrm).all())
        assert bool((res.indices >= 0).all())
        assert torch.equal(covs, sp.covariance.estimate(res.indices, P)), (k, mode, ppc)
        assert torch.equal(nrm, sp.covariance.extract_normals(P, covs)), (k, mode, ppc)
        assert torch.equal(nrm, sp.covariance.estimate_normals(res.indices, P)), (k, mode, ppc)
        _, covs2, nrm2 = grid.self_knn(k, want_knn=False, want_covs=True, want_normals=True)
        assert torch.equal(covs2, covs) and torch.equal(nrm2, nrm)
        n3 = host(nrm)[:, :3].astype(np.float64)
        assert np.abs(np.linalg.norm(n3, axis=1) - 1.0).max() <= 4 * F.EPS32
        if k >= 4:
            # the lattice plane's normals are +-e_z whatever the in-plane eigenvectors do (line and duplicates are metres away).
            # Coordinates are multiples of 1/8 below 8: every sum is exact, what is left is three roundings of the xz / yz entries
            # (|x z| <= 3.7: ~1.4e-6) against in-plane eigenvalues of at least 0.19 * 0.125^2 = 2.9e-3: a tilt below 5e-4,
            # 1 - |nz| <= 1.3e-7, and 4 eps32 for the unit length
            assert np.abs(np.abs(n3[on_plane, 2]) - 1.0).max() <= 1e-6
