"""The host twins of the photometric term (sp_intensity_gradient_host, sp_photometric_linearize_host, sp_photometric_error_host)
against the float64 model of tests/f64_photometric.py. No GPU: the twins run the per-point functions of csrc/photometric.hip on the
CPU, and tests/test_gpu_photometric.py holds the device to the twins bit for bit.

Measured here (pytest -s prints them), recorded in DESIGN.md 4.23:
  gradients, worst |d - d64| / (eps32 kappa(M) (|d64| + |g| / ||M||)) over the cases of GRADIENT_CASES: 3.71 (curved sheet; the
      textured plane stays at 0.051: its normal is an axis, so the tangent and the normal parts of M never mix)
  textured plane, interior, per-component |d - analytic|: model 0.0170 median / 0.147 maximum, twin the same to 1e-8
  term rows, worst deviation / derived bound: residual 0.015, H entries 0.14, b entries 0.015, error 0.015
"""
import ctypes as C

import numpy as np
import pytest

import f64_photometric as M
from f64_photometric import EPS32, LOSSES

NS = [1, 63, 64, 65, 1025]
KS = [2, 3, 10, 20]
# item 1: both families, the neighbourhood sizes the facade is used with
GRADIENT_CASES = [(fam, seed, k) for fam in ("plane", "sheet") for seed in (1, 2, 3) for k in (10, 20)]
GRADIENT_WORST_MEASURED = 3.71  # worst ratio of the host twin over GRADIENT_CASES, measured; the assertion allows 4 x this
GRADIENT_K = 4.0 * GRADIENT_WORST_MEASURED


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def c32(a):
    return np.ascontiguousarray(a, np.float32)


# ------------------------------------------------------------------------------------------------------------ calling the twins
def gradient_host(L, points, normals, intensities, knn):
    knn = np.ascontiguousarray(knn, np.int32)
    out = np.full((len(points), 4), 7.0, np.float32)
    rc = L.sp_intensity_gradient_host(vp(c32(points)), vp(c32(normals)), vp(c32(intensities)), len(points), vp(knn), knn.shape[1], vp(out))
    assert rc == 0, L.sp_last_error()
    return out


def photometric_params(loss="NONE", scale=1.0, max_distance=1e9, weight=1.0):
    from sycl_points_amd import _lib

    return _lib.PhotometricParams(weight, LOSSES.index(loss), scale, max_distance)


def term_host(L, case, loss="NONE", scale=1.0, max_distance=1e9, want_rows=True, error_only=False):
    """-> (sp_linearized, rows or None) of the host twin on a case dict (src, src_intensities, tgt, tgt_rows, nn_idx, nn_d2, T)"""
    from sycl_points_amd import _lib

    n = len(case["src"])
    pp = photometric_params(loss, scale, max_distance)
    out = _lib.Linearized()
    T16 = np.ascontiguousarray(np.asarray(case["T"], np.float32).T).reshape(-1)  # column-major
    head = (vp(c32(case["src"])), vp(c32(case["src_intensities"])), n, vp(c32(case["tgt"])), vp(c32(case["tgt_rows"])),
            vp(np.ascontiguousarray(case["nn_idx"], np.int32)), vp(c32(case["nn_d2"])), vp(T16), C.byref(pp), C.byref(out))
    if error_only:
        rc = L.sp_photometric_error_host(*head)
        rows = None
    else:
        rows = np.full((n, 28), 7.0, np.float32) if want_rows else None
        rc = L.sp_photometric_linearize_host(*head, vp(rows))
    assert rc == 0, L.sp_last_error()
    return out, rows


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_rows(a, b):
    """bit for bit, NaN payloads compared as 'both NaN'"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------------------------------------------------ cases
def gradient_cloud(family, n, seed):
    if family == "plane":
        return M.textured_plane(n, seed)
    return M.curved_sheet(n, seed)[:3]


def gradient_branch_case():
    """One cloud that takes every branch of the gradient row. Points 0 .. 9 lie on a 2 m grid in z = 0 with one neighbour list each:
    row 0 a full list, 1 a list with -1 entries (still >= 3 usable), 2 exactly two usable neighbours (invalid), 3 collinear
    neighbours along x (M = diag(sum x^2, 0, m^2): singular, invalid), 4 a NaN intensity of its own (invalid), 5 one neighbour with
    a NaN intensity (that neighbour is skipped; the row stays valid), 6 itself in its list (skipped), 7 a neighbour with a
    non-finite point (skipped), 8 a non-finite normal (invalid), 9 an index past the cloud (skipped)."""
    rng = np.random.RandomState(5)
    n = 24
    pts = np.ones((n, 4), np.float32)
    pts[:, :2] = rng.uniform(-3, 3, (n, 2)).astype(np.float32)
    pts[:, 2] = 0.0
    pts[10:14, :3] = np.float32([[1, 0, 0], [2, 0, 0], [-1, 0, 0], [3, 0, 0]])  # collinear with point 3 at the origin
    pts[3, :3] = 0.0
    nrm = np.zeros((n, 4), np.float32)
    nrm[:, 2] = 1.0
    inten = M.plane_intensity(pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)).astype(np.float32)
    inten[4] = np.nan
    inten[20] = np.nan
    pts[21, 0] = np.inf
    nrm[8, 1] = np.nan
    knn = np.full((n, 8), -1, np.int32)
    knn[:, :] = (np.arange(n)[:, None] + np.arange(1, 9)[None, :]) % 10 + 14  # rows default: points 14 .. 23 without 20, 21
    knn[knn == 20] = 15
    knn[knn == 21] = 16
    knn[0] = [14, 15, 16, 17, 18, 19, 22, 23]
    knn[1] = [-1, 14, -1, 15, 16, -1, 17, -1]
    knn[2] = [-1, 14, -1, 15, -1, -1, -1, -1]
    knn[3] = [10, 11, 12, 13, -1, -1, -1, -1]
    knn[5] = [14, 20, 15, 16, 17, -1, -1, -1]
    knn[6] = [6, 14, 15, 16, 6, 17, -1, -1]
    knn[7] = [14, 21, 15, 16, 17, -1, -1, -1]
    knn[9] = [14, 1000000, 15, 16, 17, -1, -1, -1]
    return pts, nrm, inten, knn


def term_case(n, seed=11):
    """a curved-sheet pair of n source points against 2 n + 50 targets with the twin's own gradient rows (filled by the caller)"""
    return M.sheet_pair(n, 2 * n + 50, seed + n)


def with_rows(L, case, k=10):
    case = dict(case)
    case["tgt_rows"] = gradient_host(L, case["tgt"], case["tgt_normals"], case["tgt_intensities"], M.knn_self(case["tgt"], k))
    return case


def branch_term_case(L, max_distance=0.25):
    """term_case(200) with every rejection planted: source 0 has index -1, 1 a distance exactly max^2 (kept), 2 the next float above
    it (rejected), 3 a target row without a gradient (w = NaN), 4 / 5 a NaN / an infinite source intensity."""
    case = with_rows(L, term_case(200))
    case["nn_d2"] = np.minimum(case["nn_d2"], np.float32(0.9 * max_distance**2)).astype(np.float32)
    max_d2 = np.float32(max_distance) * np.float32(max_distance)
    case["nn_idx"][0] = -1
    case["nn_d2"][1] = max_d2
    case["nn_d2"][2] = np.nextafter(max_d2, np.float32(np.inf))
    case["tgt_rows"][case["nn_idx"][3]] = [0.0, 0.0, 0.0, np.nan]
    case["src_intensities"][4] = np.nan
    case["src_intensities"][5] = np.inf
    hit3 = case["nn_idx"] == case["nn_idx"][3]
    rejected = np.zeros(200, bool)
    rejected[[0, 2, 4, 5]] = True
    rejected |= hit3
    return case, rejected


# ------------------------------------------------------------------------------------------------------------ bounds of item 4
def term_bounds(model, case, loss, scale):
    """Absolute bounds of one point's 28 values, residual and Jacobian, from counting roundings (u = eps32 / 2 each; constants are
    stated in eps32, i.e. with a factor 2 in hand):
      r   16 eps A, A = |d| (|R s| + |t_T| + |t|) + |I_t| + |I_s|: q = T s is four roundings per component relative to |R||s| + |t_T|
          (<= sqrt 3 of the 2-norms), e = q - t one, the dot product three relative to |d||e|, the two intensity sums one each:
          fewer than ten roundings, 10 u sqrt 3 < 9 eps.
      J   translation part v = R^T d: three roundings relative to sum |R_ij||d_i| <= sqrt 3 |d|: 3 u sqrt 3 < 4 eps |d|; rotation
          part s x v: each component two products of a coordinate of s with a component of v (error of v: 4 eps |d| each, sqrt 2 |s|
          together) and two roundings of its own relative to sqrt 2 |s||v|: < 8 eps |s||d|.
      w   the robust weight as a function of |r|: |dw/dr| <= 2 / scale for every loss (Huber 1, Tukey 1.54, Cauchy 0.65,
          Geman-McClure 0.83, all / scale), so 32 eps A / scale, plus 4 eps w for at most seven operations of its own.
      H_ac = (w J_a) J_c: w (dJ_a |J_c| + |J_a| dJ_c) + (dw + 2 eps w) |J_a J_c|      (two products: 2 u = eps, doubled)
      b_a  = (w J_a) r:   w (dJ_a |r| + |J_a| dr) + (dw + 2 eps w) |J_a r|
      e    d(error)/dr = w r for every loss: w |r| dr + 8 eps |e| (at most eight operations, powf / logf within 2 ulp), and for
           Tukey and Cauchy 4 eps scale^2: 1 - (1 - x^2)^3 and log(1 + x^2) lose the bits of x^2 below eps (absolute eps scale^2 / 6
           x 4 roundings, and eps scale^2 / 4)."""
    with np.errstate(invalid="ignore", over="ignore"):  # (rejected points may carry NaN: their bounds are never read)
        idx = np.where(case["nn_idx"] >= 0, case["nn_idx"], 0)
        d = np.linalg.norm(np.asarray(case["tgt_rows"], np.float64)[idx, :3], axis=1)
        s = np.linalg.norm(np.asarray(case["src"], np.float64)[:, :3], axis=1)
        r, J, w, A = np.abs(model["r"]), np.abs(model["J"]), model["w"], model["A"]
        dr = 16 * EPS32 * A
        dJ = 8 * EPS32 * d[:, None] * np.concatenate([np.repeat(s[:, None], 3, 1), np.ones((len(s), 3))], 1)
        dJ[:, 3:] *= 0.5
        dw = (0.0 if loss == "NONE" else 2.0 / scale * dr) + 4 * EPS32 * w
        iu = np.triu_indices(6)
        Ja, Jc, dJa, dJc = J[:, iu[0]], J[:, iu[1]], dJ[:, iu[0]], dJ[:, iu[1]]
        bH = w[:, None] * (dJa * Jc + Ja * dJc) + (dw + 2 * EPS32 * w)[:, None] * Ja * Jc
        bb = w[:, None] * (dJ * r[:, None] + J * dr[:, None]) + (dw + 2 * EPS32 * w)[:, None] * J * r[:, None]
        e = np.abs(M.robust_error(loss, r, scale))
        be = w * r * dr + 8 * EPS32 * e + (4 * EPS32 * scale**2 if loss in ("TUKEY", "CAUCHY") else 0.0)
    return dict(r=dr, J=dJ, rows=np.concatenate([bH, bb, be[:, None]], 1))


def check_rows_against_model(rows, model, bounds, what):
    """every entry of every contributing row within its bound; rejected rows exactly zero. -> worst ratios (H, b, e)"""
    m = model["mask"]
    assert (rows[~m] == 0).all(), f"{what}: a rejected point wrote something"
    dev = np.abs(rows[m].astype(np.float64) - model["rows"][m])
    ratio = dev / np.maximum(bounds["rows"][m], 1e-300)
    assert (dev <= bounds["rows"][m]).all(), f"{what}: worst deviation / bound = {ratio.max():.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return ratio[:, :21].max(initial=0.0), ratio[:, 21:27].max(initial=0.0), ratio[:, 27].max(initial=0.0)


def sum_bound(rows):
    """|float32 sum in any order - exact sum| <= (n - 1) 2^-24 sum |x_i| per column (Higham, Accuracy and Stability, 4.2, first order)"""
    n = len(rows)
    return (n - 1) * 2.0**-24 * np.abs(rows.astype(np.float64)).sum(0)


def check_sums(lin, rows, what):
    got, inlier = M.unpack_linearized(lin)
    want = rows.astype(np.float64).sum(0)
    bound = sum_bound(rows)
    assert (np.abs(got.astype(np.float64) - want) <= bound).all(), f"{what}: {np.abs(got - want)} > {bound}"
    return inlier


# ------------------------------------------------------------------------------------------------------------ 1. gradients
def test_gradients_against_the_model(L):
    """Item 1: every row of both families within K eps32 kappa(M) (|d64| + |g| / ||M||) of the float64 model, K = 4 x the measured
    worst ratio (3.71). No row is left out: every row of these clouds is valid in the model and in the twin."""
    worst = {}
    for fam, seed, k in GRADIENT_CASES:
        p, nr, it = gradient_cloud(fam, 1500, seed)
        knn = M.knn_self(p, k)
        model = M.gradient_model(p, nr, it, knn)
        got = gradient_host(L, p, nr, it, knn)
        assert model["valid"].all() and not np.isnan(got[:, 3]).any()
        assert (got[:, 3] == it).all()
        ratio = np.linalg.norm(got[:, :3].astype(np.float64) - model["rows"][:, :3], axis=1) / M.gradient_bound_unit(model)
        worst[fam] = max(worst.get(fam, 0.0), float(ratio.max()))
        assert (ratio <= GRADIENT_K).all(), (fam, seed, k, float(ratio.max()))
    print(f"\n[photometric] gradient twin vs float64, worst ratio per family: {worst} (asserted <= {GRADIENT_K})")


# ------------------------------------------------------------------------------------------------------------ 2. shapes, branches
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_gradient_shapes(L, n, k):
    """Item 2: n at the lane, wave and workgroup edges, k = 2 and 3 (at most one / two neighbours besides the point itself: every
    row invalid) and 10, 20. Validity equals the model's; valid rows within the bound of item 1."""
    p, nr, it = gradient_cloud("sheet", n, 100 + n)[:3]
    knn = M.knn_self(p, k)
    model = M.gradient_model(p, nr, it, knn)
    # a determinant within rounding of the threshold could fall on either side in float32: these clouds have none
    tie = (model["m"] >= 3) & (np.abs(np.abs(model["det"]) / M.DET_MIN - 1.0) < 1e-3)
    assert not tie.any()
    got = gradient_host(L, p, nr, it, knn)
    v = model["valid"]
    assert (np.isnan(got[:, 3]) == ~v).all()
    assert (got[~v, :3] == 0).all()
    if k <= 3 or n <= 3:
        assert not v.any()
    if v.any():
        ratio = np.linalg.norm(got[v, :3].astype(np.float64) - model["rows"][v, :3], axis=1) / M.gradient_bound_unit(model)[v]
        assert (ratio <= GRADIENT_K).all(), float(ratio.max())
        assert (got[v, 3] == it[v]).all()


def test_gradient_branches(L):
    p, nr, it, knn = gradient_branch_case()
    model = M.gradient_model(p, nr, it, knn)
    got = gradient_host(L, p, nr, it, knn)
    valid = ~np.isnan(got[:, 3])
    assert (valid == model["valid"]).all()
    assert valid[[0, 1, 5, 6, 7, 9]].all() and not valid[[2, 3, 4, 8]].any()
    assert model["m"][1] == 4 and model["m"][2] == 2 and model["m"][5] == 4 and model["m"][6] == 4 and model["m"][7] == 4 and model["m"][9] == 4
    assert model["det"][3] == 0.0  # collinear: singular exactly
    assert (got[~valid, :3] == 0).all()
    ratio = np.linalg.norm(got[valid, :3].astype(np.float64) - model["rows"][valid, :3], axis=1) / M.gradient_bound_unit(model)[valid]
    assert (ratio <= GRADIENT_K).all()


def test_constant_intensity_gives_zero_gradient_and_valid_rows(L):
    p, nr, _ = gradient_cloud("sheet", 300, 9)
    it = np.full(300, 137.25, np.float32)
    got = gradient_host(L, p, nr, it, M.knn_self(p, 10))
    assert (got[:, :3] == 0).all() and (got[:, 3] == np.float32(137.25)).all()


def test_gradient_bad_arguments(L):
    p, nr, it = gradient_cloud("plane", 8, 1)
    knn = M.knn_self(p, 4)
    out = np.zeros((8, 4), np.float32)
    assert L.sp_intensity_gradient_host(vp(p), vp(nr), vp(it), 8, vp(knn), 1, vp(out)) == 1  # k < 2
    assert b"k must be at least 2" in L.sp_last_error()
    for args in ((None, vp(nr), vp(it), 8, vp(knn), 4, vp(out)), (vp(p), None, vp(it), 8, vp(knn), 4, vp(out)),
                 (vp(p), vp(nr), None, 8, vp(knn), 4, vp(out)), (vp(p), vp(nr), vp(it), 8, None, 4, vp(out)),
                 (vp(p), vp(nr), vp(it), 8, vp(knn), 4, None)):
        assert L.sp_intensity_gradient_host(*args) == 1
    # the device entry rejects the same before any HIP call (this machine has no device to call)
    assert L.sp_intensity_gradient(vp(p), vp(nr), vp(it), 8, vp(knn), 1, vp(out), None) == 1
    assert L.sp_intensity_gradient(None, vp(nr), vp(it), 8, vp(knn), 4, vp(out), None) == 1


# ------------------------------------------------------------------------------------------------------------ 3. analytic
def test_textured_plane_gradients_against_the_analytic_ones(L):
    """Item 3: interior points (|x|, |y| < 5) of textured_plane(3000, 1), k = 10, per-component deviation from the analytic gradient.
    The model's own figures on this cloud: 0.0170 median, 0.147 maximum (the issue's prototype: 0.018 and 0.141); the twin is held
    to 1.5 x the issue's figures and to 1.5 x the model's."""
    p, nr, it = M.textured_plane(3000, 1)
    knn = M.knn_self(p, 10)
    inter = (np.abs(p[:, 0]) < 5) & (np.abs(p[:, 1]) < 5)
    ana = M.plane_intensity_gradient(p[:, 0].astype(np.float64), p[:, 1].astype(np.float64))[inter, :2]
    model = np.abs(M.gradient_model(p, nr, it, knn)["rows"][inter, :2] - ana)
    got = gradient_host(L, p, nr, it, knn)
    assert not np.isnan(got[:, 3]).any() and (got[:, 2] == 0).all()
    twin = np.abs(got[inter, :2].astype(np.float64) - ana)
    print(f"\n[photometric] |d - analytic| per component, interior: model median {np.median(model):.4f} max {model.max():.4f}; "
          f"twin median {np.median(twin):.4f} max {twin.max():.4f}; scale {np.median(np.linalg.norm(ana, axis=1)):.3f}")
    assert np.median(twin) <= 1.5 * 0.018 and twin.max() <= 1.5 * 0.141
    assert np.median(twin) <= 1.5 * np.median(model) and twin.max() <= 1.5 * model.max()


# ------------------------------------------------------------------------------------------------------------ 4. rows
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_term_rows_against_the_model(L, n):
    """Item 4: residual, Jacobian (recovered from the translation block of b and H where it can be: see below) and the 28 products
    of every point within the bounds of term_bounds. The twin does not export r and J; they are checked through the rows they
    form under LOSS_NONE (w = 1): H_33..55 = J_a J_c and b_3..5 = J_a r for the translation part, and every entry by its own bound."""
    case = with_rows(L, term_case(n))
    lin, rows = term_host(L, case)
    model = M.term_model(case["src"], case["src_intensities"], case["tgt"], case["tgt_rows"], case["nn_idx"], case["nn_d2"], case["T"])
    assert model["mask"].all()
    b = term_bounds(model, case, "NONE", 1.0)
    rH, rb, re = check_rows_against_model(rows, model, b, f"n={n}")
    # the residual through the error entry: e = r^2 / 2 exactly rounded twice, so |sqrt(2 e) - |r|| <= dr + 2 eps |r|
    r_twin = np.sqrt(2.0 * rows[:, 27].astype(np.float64))
    dev_r = np.abs(r_twin - np.abs(model["r"]))
    assert (dev_r <= b["r"] + 2 * EPS32 * np.abs(model["r"])).all()
    print(f"\n[photometric] n={n}: worst deviation / bound: r {np.max(dev_r / (b['r'] + 2 * EPS32 * np.abs(model['r']))):.3f} "
          f"H {rH:.3f} b {rb:.3f} e {re:.3f}")
    assert lin.inlier == n


# ------------------------------------------------------------------------------------------------------------ 5. branches, losses
@pytest.mark.parametrize("loss", LOSSES)
def test_term_branches_and_losses(L, loss):
    """Item 5: the rejection list (index -1, distance exactly at max^2 kept and one float past it rejected, a NaN target row, a NaN
    and an infinite source intensity), every loss at residuals on both sides of its scale, and the error entry point against the
    linearisation's error bit for bit."""
    maxd = 0.25
    case, rejected = branch_term_case(L, maxd)
    plain = M.term_model(case["src"], case["src_intensities"], case["tgt"], case["tgt_rows"], case["nn_idx"], case["nn_d2"], case["T"],
                         max_distance=maxd)
    assert (plain["mask"] == ~rejected).all() and plain["mask"][1]
    scale = float(np.median(np.abs(plain["r"][plain["mask"]])))
    a = np.abs(plain["r"][plain["mask"]])
    assert (a < 0.5 * scale).sum() > 10 and (a > 1.5 * scale).sum() > 10  # both sides of the scale
    model = M.term_model(case["src"], case["src_intensities"], case["tgt"], case["tgt_rows"], case["nn_idx"], case["nn_d2"], case["T"],
                         loss, scale, maxd)
    lin, rows = term_host(L, case, loss, scale, maxd)
    assert (rows[rejected] == 0).all() and (rows[~rejected] != 0).any(1).all()
    ratios = check_rows_against_model(rows, model, term_bounds(model, case, loss, scale), loss)
    print(f"\n[photometric] {loss}: worst deviation / bound H {ratios[0]:.3f} b {ratios[1]:.3f} e {ratios[2]:.3f}")
    assert lin.inlier == int((~rejected).sum())
    err, _ = term_host(L, case, loss, scale, maxd, error_only=True)
    assert bits(np.float32(err.error)) == bits(np.float32(lin.error)) and err.inlier == lin.inlier
    # without rows_out the sums are the same bytes
    lin2, _ = term_host(L, case, loss, scale, maxd, want_rows=False)
    assert bytes(lin2) == bytes(lin)


def test_term_bad_arguments(L):
    from sycl_points_amd import _lib

    case = with_rows(L, term_case(8))
    out = _lib.Linearized()
    T16 = np.ascontiguousarray(np.asarray(case["T"], np.float32).T).reshape(-1)
    good = [vp(c32(case["src"])), vp(c32(case["src_intensities"])), 8, vp(c32(case["tgt"])), vp(c32(case["tgt_rows"])),
            vp(np.ascontiguousarray(case["nn_idx"], np.int32)), vp(c32(case["nn_d2"])), vp(T16)]
    pp = photometric_params()
    for i in (0, 1, 3, 4, 5, 6, 7):  # every array pointer
        bad = list(good)
        bad[i] = None
        assert L.sp_photometric_linearize_host(*bad, C.byref(pp), C.byref(out), None) == 1
        assert L.sp_photometric_error_host(*bad, C.byref(pp), C.byref(out)) == 1
    assert L.sp_photometric_linearize_host(*good, None, C.byref(out), None) == 1
    assert L.sp_photometric_linearize_host(*good, C.byref(pp), None, None) == 1
    for bad_pp in (photometric_params("HUBER", 0.0), photometric_params("CAUCHY", -1.0), photometric_params("TUKEY", float("nan"))):
        assert L.sp_photometric_linearize_host(*good, C.byref(bad_pp), C.byref(out), None) == 1
        assert b"robust_scale" in L.sp_last_error()
    for t in (-1, 5):
        bad_pp = photometric_params()
        bad_pp.robust_type = t
        assert L.sp_photometric_linearize_host(*good, C.byref(bad_pp), C.byref(out), None) == 1
    # the device entries reject the same, and a null, short or misaligned workspace, before any HIP call
    ws = np.zeros(L.sp_photometric_workspace_bytes(8) + 64, np.uint8)
    base = ws.ctypes.data + (-ws.ctypes.data) % 16
    dev = lambda w, nbytes, p=pp: L.sp_photometric_linearize(*good, 0, C.byref(p), C.byref(out), None, w, nbytes, None)  # noqa: E731
    assert dev(None, ws.size) == 1 and dev(C.c_void_p(base), 1024) == 1 and dev(C.c_void_p(base + 4), ws.size - 16) == 1
    assert dev(C.c_void_p(base), ws.size - 16, photometric_params("HUBER", 0.0)) == 1
    assert L.sp_photometric_error(*good, 0, C.byref(pp), C.byref(out), None, ws.size, None) == 1
    assert L.sp_photometric_workspace_bytes(8) == L.sp_photometric_workspace_bytes(1 << 20) > 0
    # n == 0 on the host: zeros
    out.error = 3.0
    assert L.sp_photometric_linearize_host(None, None, 0, None, None, None, None, vp(T16), C.byref(pp), C.byref(out), None) == 0
    assert out.error == 0.0 and out.inlier == 0


# ------------------------------------------------------------------------------------------------------------ 6. sums
@pytest.mark.parametrize("n", [1, 65, 1025, 4099])
def test_term_sums(L, n):
    """Item 6: the twin's sums against the float64 sum of the twin's own rows, within (n - 1) 2^-24 sum |row entries| per entry;
    inlier exact."""
    case = with_rows(L, term_case(n))
    case["nn_idx"][::7] = -1  # some rejected points among them
    lin, rows = term_host(L, case, "CAUCHY", 5.0)
    inlier = check_sums(lin, rows, f"n={n}")
    assert inlier == lin.inlier == n - len(range(0, n, 7))
    H = np.array(lin.H, np.float32).reshape(6, 6)
    assert (H == H.T).all() and lin.inlier_hi * 4096 + lin.inlier_lo == lin.inlier
