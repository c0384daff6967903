"""The photometric term on the device (csrc/photometric.hip) against its host twins, bit for bit, and end to end through
api.Registration.align and the C++ facade (tests/cpp/test_photometric.cpp). The twins are held to the float64 model by
tests/test_photometric_cpu.py, whose cases, bounds and helpers this file uses.

Measured on an MI355X (pytest -s prints them), recorded in DESIGN.md 4.23 (errors: translation / Frobenius norm of the rotation
difference):
  textured plane (target 3000, source 1500 points, yaw 2 degrees, t = (0.3, -0.2, 0.05), POINT_TO_PLANE, k = 10, max distance 1.5):
    float64 aligner (the yardstick), weight 25: 4.851e-4 m / 1.265e-4 (the issue's prototype, another sample: 1.0e-3 / 4.4e-4)
    weight 0: in-plane error 0.3606 m, rotation 0.0494 (where it started; only z is recovered)
    weight 25: GN 4.885e-4 m / 1.253e-4, LM 4.885e-4 / 1.253e-4, DOGLEG 4.883e-4 / 1.253e-4, GN + NL_REG 4.885e-4 / 1.253e-4, each
    converged in 2 iterations; the C++ facade the same
  bundled pair (6122 / 6094 points, weight 1.82e-8): geometry only 9.169e-3 m / 5.983e-3, with the term 9.172e-3 m / 5.976e-3
  device rows_out against the host twin: equal bits under every loss (with sp_math.h's robust_error, whose Tukey and Cauchy errors
    call powf / logf, the error entry alone differed: up to 1166 of 4099 rows, 2 - 5 ulp Cauchy, up to 2023 ulp Tukey)
"""
import os
import subprocess

import numpy as np
import pytest

import f64_photometric as M
import test_photometric_cpu as H
from f64_photometric import LOSSES

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CPP = os.path.join(ROOT, "tests", "cpp")
TERM_NS = [1, 63, 64, 65, 1025, 4099]


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cloud(sp, points, normals=None, intensities=None):
    return sp.PointCloudShared(dev(H.c32(points)), normals=None if normals is None else dev(H.c32(normals)),
                               intensities=None if intensities is None else dev(H.c32(intensities)))


def gradient_dev(sp, points, normals, intensities, knn):
    rows = sp.intensity_gradients(dev(np.ascontiguousarray(knn, np.int32)), cloud(sp, points, normals, intensities))
    torch.cuda.synchronize()
    return rows.cpu().numpy()


def neighbors_of(sp, case):
    nn = sp.KNNResult()
    n = len(case["src"])
    nn.indices, nn.distances = dev(np.ascontiguousarray(case["nn_idx"], np.int32).reshape(n, 1)), dev(H.c32(case["nn_d2"]).reshape(n, 1))
    nn.query_size, nn.k = n, 1
    return nn


def term_dev(sp, case, loss="NONE", scale=1.0, max_distance=1e9, T_on_device=False, want_rows=True, error_only=False, repeat=1):
    """-> list over `repeat` launches of (Linearized, rows or None)"""
    src = cloud(sp, case["src"], intensities=case["src_intensities"])
    tgt, rows_t, nn = dev(H.c32(case["tgt"])), dev(H.c32(case["tgt_rows"])), neighbors_of(sp, case)
    T = np.asarray(case["T"], np.float32)
    Targ = dev(np.ascontiguousarray(T.T).reshape(-1)) if T_on_device else T
    pp = sp.PhotometricParams(weight=1.0, robust_type=loss, robust_scale=scale)
    out = []
    for _ in range(repeat):
        if error_only:
            lin, rows = sp.photometric_error(src, tgt, rows_t, nn, Targ, pp, max_distance), None
        elif want_rows:
            lin, rows = sp.photometric_linearize(src, tgt, rows_t, nn, Targ, pp, max_distance, want_rows=True)
        else:
            lin, rows = sp.photometric_linearize(src, tgt, rows_t, nn, Targ, pp, max_distance), None
        torch.cuda.synchronize()
        out.append((sp.Registration._read_lin(lin), None if rows is None else rows.cpu().numpy()))
    return out


_cases = {}


def term_case(L, n):
    if n not in _cases:
        _cases[n] = H.with_rows(L, H.term_case(n))
    return _cases[n]


# ------------------------------------------------------------------------------------------------------------ 7. gradients
def test_gradient_rows_are_the_twins_bits(sp, L):
    """Item 7: every shape and case of items 1 and 2 of the CPU suite, NaN payloads compared as 'both NaN'."""
    clouds = [H.gradient_cloud(fam, 1500, seed) + (k,) for fam, seed, k in H.GRADIENT_CASES]
    clouds += [H.gradient_cloud("sheet", n, 100 + n) + (k,) for n in H.NS for k in H.KS]
    for p, nr, it, k in clouds:
        knn = M.knn_self(p, k)
        assert H.same_rows(gradient_dev(sp, p, nr, it, knn), H.gradient_host(L, p, nr, it, knn)), (len(p), k)
    p, nr, it, knn = H.gradient_branch_case()
    got = gradient_dev(sp, p, nr, it, knn)
    assert H.same_rows(got, H.gradient_host(L, p, nr, it, knn))
    assert np.isnan(got[[2, 3, 4, 8], 3]).all() and not np.isnan(got[[0, 1, 5, 6, 7, 9], 3]).any()
    p, nr, _ = H.gradient_cloud("sheet", 300, 9)
    it = np.full(300, 137.25, np.float32)
    got = gradient_dev(sp, p, nr, it, M.knn_self(p, 10))
    assert (got[:, :3] == 0).all() and (got[:, 3] == np.float32(137.25)).all()
    # k > 64 and a neighbour array that is not 16-byte aligned take the kernel without the staged index lists: the same bits
    p, nr, it = H.gradient_cloud("sheet", 300, 10)
    knn = M.knn_self(p, 70)
    assert H.same_rows(gradient_dev(sp, p, nr, it, knn), H.gradient_host(L, p, nr, it, knn))
    knn = M.knn_self(p, 10)
    buf = torch.zeros(300 * 10 + 1, dtype=torch.int32, device="cuda")
    buf[1:] = dev(knn).reshape(-1)
    rows = sp.intensity_gradients(buf[1:].view(300, 10), cloud(sp, p, nr, it))
    torch.cuda.synchronize()
    assert H.same_rows(rows.cpu().numpy(), H.gradient_host(L, p, nr, it, knn))


def test_gradient_errors(sp):
    p, nr, it = H.gradient_cloud("plane", 64, 1)
    knn = dev(M.knn_self(p, 10))
    with pytest.raises(sp.SpError):
        sp.intensity_gradients(knn, cloud(sp, p, None, it))
    with pytest.raises(sp.SpError):
        sp.intensity_gradients(knn, cloud(sp, p, nr, None))
    with pytest.raises(sp.SpError):
        sp.intensity_gradients(knn[:, :1].contiguous(), cloud(sp, p, nr, it))  # k < 2


# ------------------------------------------------------------------------------------------------------------ 8. rows
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("n", TERM_NS)
def test_term_rows_are_the_twins_bits(sp, L, n, loss):
    """Item 8: rows_out of the device = rows of the host twin, bit for bit, for every loss, with the pose on the host and on the
    device; some points rejected, so that zero rows occur."""
    case = dict(term_case(L, n))
    case["nn_idx"] = case["nn_idx"].copy()
    case["nn_idx"][3::11] = -1
    plain = M.term_model(case["src"], case["src_intensities"], case["tgt"], case["tgt_rows"], case["nn_idx"], case["nn_d2"], case["T"])
    scale = float(np.median(np.abs(plain["r"]))) if loss != "NONE" else 1.0
    _, want = H.term_host(L, case, loss, scale)
    for on_device in (False, True):
        (lin, rows), = term_dev(sp, case, loss, scale, T_on_device=on_device)
        diff = H.bits(rows) != H.bits(want)
        assert not diff.any(), (f"T_on_device={on_device}: {int(diff.sum())} entries differ, columns {sorted(set(np.nonzero(diff)[1].tolist()))}, "
                                f"worst ulp {int(np.abs(H.bits(rows).astype(np.int64) - H.bits(want).astype(np.int64)).max())}")
        assert lin.inlier == n - len(range(3, n, 11))


# ------------------------------------------------------------------------------------------------------------ 9. sums
@pytest.mark.parametrize("n", TERM_NS)
def test_term_sums(sp, L, n):
    """Item 9: the device's sums against the float64 sum of its own rows (the bound of item 6), the exact count, a second launch
    with the same bytes, the error entry point, and a launch in which every point is rejected."""
    case = dict(term_case(L, n))
    case["nn_idx"] = case["nn_idx"].copy()
    case["nn_idx"][::7] = -1
    (lin, rows), (lin2, rows2) = term_dev(sp, case, "CAUCHY", 5.0, repeat=2)
    inlier = H.check_sums(lin, rows, f"n={n}")
    assert inlier == lin.inlier == n - len(range(0, n, 7)) and lin.inlier_hi * 4096 + lin.inlier_lo == lin.inlier
    assert bytes(lin2) == bytes(lin) and rows2.tobytes() == rows.tobytes()
    (lin3, _), = term_dev(sp, case, "CAUCHY", 5.0, want_rows=False)
    assert bytes(lin3) == bytes(lin)
    (err, _), = term_dev(sp, case, "CAUCHY", 5.0, error_only=True)
    assert H.bits(np.float32(err.error)) == H.bits(np.float32(lin.error)) and err.inlier == lin.inlier
    case["nn_idx"][:] = -1
    (none, rows0), = term_dev(sp, case, "CAUCHY", 5.0)
    assert bytes(none) == bytes(192) and not rows0.any()
    (none, _), = term_dev(sp, case, "CAUCHY", 5.0, error_only=True)
    assert none.error == 0.0 and none.inlier == 0


def test_term_bad_arguments_on_the_device(sp, L):
    case = term_case(L, 65)
    with pytest.raises(sp.SpError):
        term_dev(sp, case, "HUBER", 0.0)
    src = cloud(sp, case["src"], intensities=case["src_intensities"])
    small = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    with pytest.raises(sp.SpError):
        sp.photometric_linearize(src, dev(case["tgt"]), dev(case["tgt_rows"]), neighbors_of(sp, case), case["T"], sp.PhotometricParams(), 1.0,
                                 workspace=small)


# ------------------------------------------------------------------------------------------------------------ 10. end to end
def plane_clouds(sp):
    sc = M.plane_scene()
    source = cloud(sp, sc["src"], sc["src_normals"], sc["src_intensities"])
    target = cloud(sp, sc["tgt"], sc["tgt_normals"], sc["tgt_intensities"])
    tree = sp.KDTree.build(target.points)
    grads = sp.intensity_gradients(tree.knn_search(target, 10), target)
    return sc, source, target, tree, grads


# NL-Reg calls a direction weak when its eigenvalue of H per inlier is below a threshold (defaults 10 / 1, set for geometric
# factors) and then ties it to the initial pose. Geometry alone gives the plane's three free directions an eigenvalue of 0; the
# photometric term gives them weight x E[d^2] per inlier = 25 x 0.025 .. 0.077 = 0.6 .. 1.9 (translation) and about 30 (yaw). With
# the thresholds a tenth of the defaults the geometric system alone is still held at the initial pose (asserted below) and the
# combined system is not: the bound of the other optimisers holds only if the regulariser sees the combined system.
NL_REG = dict(degenerate_reg_type="NL_REG", degenerate_reg_rot_eigenvalue_threshold=1.0, degenerate_reg_trans_eigenvalue_threshold=0.1)


def plane_params(sp, weight, method="GN", **kw):
    """POINT_TO_PLANE, k = 10 gradients, max distance 1.5; everything else the defaults (criteria 1e-3)"""
    return sp.RegistrationParams(reg_type="POINT_TO_PLANE", max_correspondence_distance=1.5, max_iterations=30, optimization_method=method,
                                 photometric=sp.PhotometricParams(weight=weight), **kw)


@pytest.fixture(scope="module")
def yardstick():
    sc = M.plane_scene()
    T, used = M.align_f64(sc["src"], sc["src_intensities"], sc["tgt"], sc["tgt_normals"], sc["tgt_intensities"], 25.0, k=10, max_distance=1.5)
    _, t, r = M.pose_errors(T)
    print(f"\n[photometric] float64 aligner, weight 25: {t:.3e} m / {r:.3e} in {used} iterations")
    return t, r


def test_weight_zero_is_the_existing_align(sp):
    """Item 10: with weight 0 the call that takes gradients returns the bytes of the call that does not, and the pose stays where
    geometry leaves it: more than 0.3 m off in the plane (0.361 in the model)."""
    _, source, target, tree, grads = plane_clouds(sp)
    a = sp.Registration(plane_params(sp, 0.0)).align(source, target, tree)
    b = sp.Registration(plane_params(sp, 0.0)).align(source, target, tree, target_gradients=grads)
    for f in ("T", "H", "b", "H_raw", "b_raw"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert (a.error, a.inlier, a.iterations, a.converged) == (b.error, b.inlier, b.iterations, b.converged)
    in_plane, _, rot = M.pose_errors(b.T)
    print(f"\n[photometric] weight 0: in-plane error {in_plane:.4f} m, rotation {rot:.4f}")
    assert in_plane > 0.3


@pytest.mark.parametrize("method,reg", [("GN", "NONE"), ("LM", "NONE"), ("DOGLEG", "NONE"), ("GN", "NL_REG")])
def test_textured_plane_alignment(sp, yardstick, method, reg):
    """Item 10: weight 25 under each optimiser, and with the degenerate regulariser on (it must see the combined system): converged,
    translation and rotation errors within 3 x the float64 aligner's on the same clouds (4.85e-4 m / 1.27e-4; the issue's prototype:
    1.0e-3 / 4.4e-4). The factor 3 is room for float32 sums and for other nearest-neighbour ties, nothing else."""
    _, source, target, tree, grads = plane_clouds(sp)
    kw = NL_REG if reg == "NL_REG" else {}
    res = sp.Registration(plane_params(sp, 25.0, method, **kw)).align(source, target, tree, target_gradients=grads)
    _, t, r = M.pose_errors(res.T)
    print(f"\n[photometric] {method} {reg}: {t:.3e} m / {r:.3e} ({res.iterations} iterations, converged {res.converged}, "
          f"{res.inlier} inliers); yardstick {yardstick[0]:.3e} / {yardstick[1]:.3e}")
    assert res.converged
    assert t <= 3.0 * yardstick[0] and r <= 3.0 * yardstick[1]
    assert 0 < res.inlier <= source.size()
    assert res.H_raw.tobytes() != np.zeros((6, 6), np.float32).tobytes()
    if reg == "NL_REG":  # the same regulariser on geometry alone holds the plane's free directions at the initial pose
        alone = sp.Registration(plane_params(sp, 0.0, method, **NL_REG)).align(source, target, tree)
        assert M.pose_errors(alone.T)[0] > 0.3 and np.trace(alone.H - alone.H_raw) > 1000.0  # (three weak directions x 1500 inliers)


def test_cpp_facade(sp, yardstick, tmp_path):
    """Item 10 / 11 through the C++ facade (tests/cpp/test_photometric.cpp, built here with the facade tests' flags)."""
    from test_gpu_lidar_odometry import build

    exe = build(os.path.join(CPP, "test_photometric.cpp"), os.path.join(CPP, "test_photometric"))
    sc = M.plane_scene()
    path = str(tmp_path / "plane.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(sc["src"]), len(sc["tgt"])], np.int32).tobytes())
        for c in ("src", "tgt"):
            f.write(H.c32(sc[c]).tobytes())
            f.write(H.c32(sc[c + "_normals"]).tobytes())
            f.write(H.c32(sc[c + "_intensities"]).tobytes())
    r = subprocess.run([exe, path, repr(yardstick[0]), repr(yardstick[1])], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout[-4000:]
    for name in ("gradients", "weight_zero", "optimizers", "degenerate", "error_paths"):
        assert f"[  OK  ] {name}" in r.stdout, name


# ------------------------------------------------------------------------------------------------------------ 11. error paths
def test_align_error_paths(sp):
    """Item 11 in the mirror (the communicator is the facade's: tests/cpp/test_photometric.cpp): no source intensities and a size
    mismatch raise before anything is enqueued."""
    sc, source, target, tree, grads = plane_clouds(sp)
    reg = sp.Registration(plane_params(sp, 25.0))
    with pytest.raises(sp.SpError):
        reg.align(cloud(sp, sc["src"], sc["src_normals"]), target, tree, target_gradients=grads)
    with pytest.raises(sp.SpError):
        reg.align(source, target, tree, target_gradients=grads[:-1].contiguous())
    assert reg.neighbors.indices is None  # nothing was searched, nothing enqueued
    assert reg.align(source, target, tree, target_gradients=grads).converged


# ------------------------------------------------------------------------------------------------------------ 12. bundled pair
def test_bundled_pair_is_not_harmed(sp):
    """Item 12: the bundled scans carry scalar_intensity. Box filter [0.5, 50] m, 0.25 m voxels, k = 10 covariances and normals; GICP
    with and without the term, weight = 1e-4 x trace(H geometric) / trace(H photometric) at the identity. Real intensities are
    noisy: asserted is only that the result is finite, converged and no further from T_target_source than 2 x the geometry-only
    result."""
    from test_sampling_cpu import read_ply_xyzi

    def prep(name):
        raw = read_ply_xyzi(os.path.join(GOLD, name))
        rng = np.linalg.norm(raw[:, :3], axis=1)
        raw = raw[(rng >= 0.5) & (rng <= 50.0)]
        pts = np.ones((len(raw), 4), np.float32)
        pts[:, :3] = raw[:, :3]
        c = sp.VoxelGrid(0.25).downsampling(sp.PointCloudShared(dev(pts), intensities=dev(np.ascontiguousarray(raw[:, 3]))))
        assert c.has_intensity()
        tree = sp.KDTree.build(c.points)
        nn = tree.knn_search(c, 10)
        sp.covariance.estimate(nn, c)
        sp.covariance.estimate_normals(nn, c)
        return c, tree, nn

    (source, _, _), (target, tree, nn) = prep("source.ply"), prep("target.ply")
    T_gt = np.loadtxt(os.path.join(GOLD, "T_target_source.txt"))
    grads = sp.intensity_gradients(nn, target)
    valid = int((~torch.isnan(grads[:, 3])).sum())
    params = lambda w: sp.RegistrationParams(reg_type="GICP", max_correspondence_distance=2.0, max_iterations=30,  # noqa: E731
                                             photometric=sp.PhotometricParams(weight=w))
    reg = sp.Registration(params(0.0))
    geo = reg.compute_linearized_result(source, target, tree, np.eye(4, dtype=np.float32))
    pho = sp.Registration._read_lin(sp.photometric_linearize(source, target.points, grads, reg.neighbors, np.eye(4, dtype=np.float32),
                                                             sp.PhotometricParams(), 2.0))
    tr_pho = float(np.trace(np.array(pho.H, np.float32).reshape(6, 6)))
    assert pho.inlier > 0 and tr_pho > 0
    weight = 1e-4 * float(np.trace(geo["H"])) / tr_pho
    plain = sp.Registration(params(0.0)).align(source, target, tree)
    both = sp.Registration(params(weight)).align(source, target, tree, target_gradients=grads)

    def errs(T):
        d = np.asarray(T, np.float64) - T_gt
        return float(np.linalg.norm(d[:3, 3])), float(np.linalg.norm(d[:3, :3]))

    (gt, gr), (pt, pr) = errs(plain.T), errs(both.T)
    print(f"\n[photometric] bundled pair: {source.size()} source / {target.size()} target points, {valid} target rows with a gradient, "
          f"weight {weight:.4e}; geometry only {gt:.3e} m / {gr:.3e} ({plain.iterations} it); with the term {pt:.3e} m / {pr:.3e} "
          f"({both.iterations} it, converged {both.converged})")
    assert np.isfinite(both.T).all() and both.converged
    assert pt <= 2.0 * gt and pr <= 2.0 * gr
