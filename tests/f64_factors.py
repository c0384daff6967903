"""A float64 model of the linearised registration system for every factor and every robust loss, written FROM THE MATHEMATICS
(tests/test_oracle_gicp_f64.py says why: kernels and oracle were written from the same reading of factor.hpp, so "GPU == oracle"
alone could hide an error both share). A plain helper module shared by tests/test_oracle_factors_f64.py (the oracle, no GPU) and
tests/test_gpu_factors_f64.py (the kernels).

Per correspondence (source point p, target point q, pose T = [R | t]):

    r(T) = q - T p
    e(T) = r^T M r                      M frozen at the linearisation pose (which is what Gauss-Newton linearises)
    M    = I                            POINT_TO_POINT
         = n n^T                        POINT_TO_PLANE, n the UNIT target normal
         = Ct^-1                        POINT_TO_DISTRIBUTION
         = (plane(Ct) + R plane(Cs) R^T)^-1,  plane(C) = V diag(1e-3, 1, 1) V^T      GICP (Segal et al.)
         = n n^T when lambda0 / sum(lambda) of Ct is below 0.2, else I               GENZ (Lee et al., arXiv 2411.06766)
    g    = alpha for a planar GENZ correspondence, 1 - alpha for the others; 1 for every other factor
    cost = g rho(sqrt(e), s)

    rho(r, s) = r^2 / 2                                               NONE
              = r^2 / 2 (r <= s),  s (r - s / 2) (r > s)              HUBER
              = s^2 / 6 (1 - (1 - r^2 / s^2)^3) (r <= s),  s^2 / 6    TUKEY
              = s^2 / 2 log(1 + r^2 / s^2)                            CAUCHY
              = s^2 r^2 / (2 (s^2 + r^2))                             GEMAN_MCCLURE

Summed over the inlier correspondences (d2 <= max_corr^2):

    error = sum g rho(sqrt(e))
    b     = d/d(delta) sum cost(T exp(delta))    central finite difference, delta = [rotation(3), translation(3)]
    H     = sum g w J^T M J,   J = dr/d(delta) by central differences of the residual,
                               w = rho'(r) / r by a central difference of rho (NOT the closed-form IRLS weight)

exp() is scipy's matrix exponential of the 4x4 twist matrix. Nothing in system_fd() builds a Jacobian analytically; system_fast()
is the same sum with J = [R skew(p) | -R] for the size sweeps, and tests/test_oracle_factors_f64.py holds it to system_fd() before
anything else uses it.

make_case() builds inputs on which nothing discontinuous sits near its threshold (its docstring lists how), so that a float32
implementation and this model cannot fall on different sides of a branch.
"""
import numpy as np
from scipy.linalg import expm

FACTORS = ("POINT_TO_POINT", "POINT_TO_PLANE", "POINT_TO_DISTRIBUTION", "GICP", "GENZ")
LOSSES = ("NONE", "HUBER", "TUKEY", "CAUCHY", "GEMAN_MCCLURE")
GENZ_THRESHOLD = 0.2       # registration_params.hpp: genz.planarity_threshold
GENZ_ALPHA = 0.7           # what the tests hand to oracle and kernels (not 0.5: planar and non-planar weights differ)
MAX_CORR = 2.0
REJECTED_D2 = 100.0        # > MAX_CORR^2 by a wide margin: the inlier gate is never decided by rounding
FD_STEP = 1e-6
GENERATING_TWIST = np.array([0.01, -0.02, 0.015, 0.03, -0.02, 0.01])


def twist_matrix(d):
    w, v = d[:3], d[3:]
    X = np.zeros((4, 4))
    X[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    X[:3, 3] = v
    return X


def plane(C):
    """V diag(1e-3, 1, 1) V^T, the smallest eigenvalue's direction squeezed; C: (..., 3, 3)."""
    _, V = np.linalg.eigh(C)  # ascending
    return np.einsum("...ik,k,...jk->...ij", V, np.array([1e-3, 1.0, 1.0]), V)


def curvature(C):
    lam = np.linalg.eigvalsh(C)
    return lam[..., 0] / lam.sum(axis=-1)


def rho(loss, r, s):
    r = np.asarray(r, np.float64)
    if loss == "NONE":
        return 0.5 * r * r
    if loss == "HUBER":
        return np.where(r <= s, 0.5 * r * r, s * (r - 0.5 * s))
    if loss == "TUKEY":
        return np.where(r <= s, s * s / 6.0 * (1.0 - (1.0 - np.minimum(r / s, 1.0) ** 2) ** 3), s * s / 6.0)
    if loss == "CAUCHY":
        return 0.5 * s * s * np.log1p(r * r / (s * s))
    if loss == "GEMAN_MCCLURE":
        return 0.5 * s * s * r * r / (s * s + r * r)
    raise ValueError(loss)


def irls_weight_fd(loss, r, s):
    """w = rho'(r) / r with rho' a central difference of rho."""
    h = FD_STEP * s
    return (rho(loss, r + h, s) - rho(loss, r - h, s)) / (2.0 * h * r)


def cov3(covs16):
    """float[16] column-major 4x4 -> float64 3x3 blocks."""
    return np.asarray(covs16).reshape(-1, 4, 4).transpose(0, 2, 1)[:, :3, :3].astype(np.float64)


def cov16(C):
    out = np.zeros((len(C), 4, 4), np.float32)
    out[:, :3, :3] = C
    return np.ascontiguousarray(out.transpose(0, 2, 1)).reshape(-1, 16)


class Case:
    """The float32 arrays oracle and kernels are given; the model reads the same values, widened to float64."""

    def __init__(self, src, scov, tgt, tcov, nrm, nn, d2, T):
        self.src, self.scov, self.tgt, self.tcov, self.nrm = src, scov, tgt, tcov, nrm
        self.nn, self.d2, self.T = nn, d2, T
        self.max_corr, self.alpha = MAX_CORR, GENZ_ALPHA

    @property
    def inliers(self):
        mc = np.float32(self.max_corr)
        return self.d2 <= mc * mc  # in float32, as registration.hpp:593-596 gates

    def with_correspondences(self, nn, d2):
        return Case(self.src, self.scov, self.tgt, self.tcov, self.nrm, np.ascontiguousarray(nn, np.int32),
                    np.ascontiguousarray(d2, np.float32), self.T)

    def with_pose(self, T):
        return Case(self.src, self.scov, self.tgt, self.tcov, self.nrm, self.nn, self.d2, np.asarray(T, np.float32))


def random_rotations(rs, n):
    q, r = np.linalg.qr(rs.normal(size=(n, 3, 3)))
    q = q * np.sign(np.einsum("nii->ni", r))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    return q


def synthetic_covariances(rs, n):
    """V diag(lambda) V^T with a random rotation V, even rows planar (lambda0 / sum <= 0.05), odd rows blobs (>= 0.28): the GENZ
    class is decided far from 0.2. A blob's eigenvalues are as far apart as curvature >= 0.28 lets them be (1 : 1.18 : 1.36, each
    covariance scaled by a random factor in [1, 2]): a float32 eigenvector is off by rounding / eigenvalue gap, and GICP's plane()
    needs all three; every determinant is >= 4e-6 (eigen_utils::inverse returns Zero below 1e-6). Returns the float32-rounded
    matrices as float64 (exactly symmetric) and the unit eigenvector of the smallest eigenvalue."""
    f = rs.uniform(1.0, 2.0, n)
    lam = np.empty((n, 3))
    planar = np.arange(n) % 2 == 0
    lam[:] = np.where(planar[:, None], [0.004, 0.090, 0.150], [0.0300, 0.0354, 0.0408])  # curvature 0.016 and 0.2825
    lam *= f[:, None]
    V = random_rotations(rs, n)
    C = np.einsum("nik,nk,njk->nij", V, lam, V)
    C = (0.5 * (C + C.transpose(0, 2, 1))).astype(np.float32).astype(np.float64)
    c = curvature(C)
    assert (c[planar] <= 0.05).all() and (c[~planar] >= 0.28).all(), "the GENZ class must be decided far from 0.2"
    assert (np.linalg.det(C) >= 4e-6).all(), "determinants must stay far above eigen_utils::inverse's 1e-6"
    return C, V[:, :, 0]


def make_case(n_src, n_tgt, seed=20240611, reject_every=7, reject_from=3, noise=0.02):
    """Fixed-seed inputs on which nothing discontinuous sits near its threshold:
    * covariances given directly (synthetic_covariances; no KNN), the target normal the UNIT eigenvector of the smallest eigenvalue —
      POINT_TO_PLANE's M = n n^T assumes unit normals (non-unit normals are outside what these tests cover);
    * correspondences and squared distances are inputs: source i was generated from target nn[i] (T_gen^-1 q + noise), every
      `reject_every`-th correspondence from index `reject_from` on is rejected with d2 = 100 (reject_every 0: none);
    * the pose is half of the generating motion, so that b is not ~ 0;
    * the cloud sits off the origin, so that no 3x3 block of H is a sum that cancels."""
    rs = np.random.RandomState(seed)
    tgt = np.ones((n_tgt, 4), np.float32)
    tgt[:, :3] = rs.uniform(0.0, 8.0, (n_tgt, 3)) + np.array([1.0, -2.0, 0.5])
    Ct, normal = synthetic_covariances(rs, n_tgt)
    Cs, _ = synthetic_covariances(rs, n_src)
    nrm = np.zeros((n_tgt, 4), np.float32)
    nrm[:, :3] = normal
    nn = rs.randint(0, n_tgt, n_src).astype(np.int32)
    Tg = np.linalg.inv(expm(twist_matrix(GENERATING_TWIST)))
    src = np.ones((n_src, 4), np.float32)
    src[:, :3] = tgt[nn, :3].astype(np.float64) @ Tg[:3, :3].T + Tg[:3, 3] + rs.normal(0.0, noise, (n_src, 3))
    T = expm(0.5 * twist_matrix(GENERATING_TWIST)).astype(np.float32)
    q = src[:, :3].astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)
    d2 = ((tgt[nn, :3].astype(np.float64) - q) ** 2).sum(axis=1).astype(np.float32)
    assert d2.max() < 0.25 * MAX_CORR ** 2
    if reject_every:
        d2[reject_from::reject_every] = REJECTED_D2
    return Case(src, cov16(Cs), tgt, cov16(Ct), nrm, nn, d2, T)


def _geometry(case, factor):
    """Per inlier correspondence: p, q, M (frozen at case.T), g; all float64."""
    inl = np.flatnonzero(case.inliers)
    T = case.T.astype(np.float64)
    R = T[:3, :3]
    p = case.src[inl, :3].astype(np.float64)
    j = case.nn[inl]
    q = case.tgt[j, :3].astype(np.float64)
    m = len(inl)
    eye = np.broadcast_to(np.eye(3), (m, 3, 3))
    g = np.ones(m)
    if factor == "POINT_TO_POINT":
        M = eye
    elif factor in ("POINT_TO_PLANE", "GENZ"):
        n = case.nrm[j, :3].astype(np.float64)
        nnT = np.einsum("ni,nj->nij", n, n)
        if factor == "POINT_TO_PLANE":
            M = nnT
        else:
            c = curvature(cov3(case.tcov[j]))
            assert (np.abs(c - GENZ_THRESHOLD) > 0.05).all()
            planar = c < GENZ_THRESHOLD
            M = np.where(planar[:, None, None], nnT, eye)
            g = np.where(planar, case.alpha, 1.0 - case.alpha)
    elif factor == "POINT_TO_DISTRIBUTION":
        M = np.linalg.inv(cov3(case.tcov[j]))
    elif factor == "GICP":
        M = np.linalg.inv(plane(cov3(case.tcov[j])) + R @ plane(cov3(case.scov[inl])) @ R.T)
    else:
        raise ValueError(factor)
    return inl, T, p, q, M, g


def _residuals(T, p, q):
    return q - (p @ T[:3, :3].T + T[:3, 3])


def residual_norms(case, factor, T=None):
    """sqrt(e) of every inlier at pose T (default: the linearisation pose), M frozen at case.T."""
    _, T0, p, q, M, _ = _geometry(case, factor)
    r = _residuals(T0 if T is None else np.asarray(T, np.float64), p, q)
    return np.sqrt(np.einsum("ni,nij,nj->n", r, M, r))


def robust_scale(case, factor):
    """The float32-rounded median of the inliers' residual norms: both branches of HUBER and of TUKEY are populated. All five
    losses are continuous at the scale, so no point needs excluding."""
    rn = residual_norms(case, factor)
    s = float(np.float32(np.median(rn)))
    assert (rn < s).mean() >= 0.25 and (rn > s).mean() >= 0.25, "at least a quarter of the inliers on each side of the scale"
    return s


def system_fd(case, factor, loss, scale):
    """error, b, H and the per-inlier w, all by finite differences (see the module docstring); no analytic Jacobian."""
    inl, T, p, q, M, g = _geometry(case, factor)
    h = FD_STEP
    b = np.zeros(6)
    J = np.zeros((len(inl), 3, 6))
    for a in range(6):
        d = np.zeros(6)
        d[a] = h
        rp = _residuals(T @ expm(twist_matrix(d)), p, q)
        rm = _residuals(T @ expm(twist_matrix(-d)), p, q)
        cp = g * rho(loss, np.sqrt(np.einsum("ni,nij,nj->n", rp, M, rp)), scale)
        cm = g * rho(loss, np.sqrt(np.einsum("ni,nij,nj->n", rm, M, rm)), scale)
        b[a] = (cp.sum() - cm.sum()) / (2 * h)
        J[:, :, a] = (rp - rm) / (2 * h)
    r0 = _residuals(T, p, q)
    rn = np.sqrt(np.einsum("ni,nij,nj->n", r0, M, r0))
    w = irls_weight_fd(loss, rn, scale)
    H = np.einsum("n,nia,nij,njb->ab", g * w, J, M, J)
    return {"H": H, "b": b, "error": float((g * rho(loss, rn, scale)).sum()), "inlier": len(inl), "w": w, "index": inl}


def system_fast(case, factor, loss, scale):
    """The same sums with J = [R skew(p) | -R] (held to system_fd by tests/test_oracle_factors_f64.py): for the size sweeps."""
    inl, T, p, q, M, g = _geometry(case, factor)
    R = T[:3, :3]
    S = np.zeros((len(inl), 3, 3))
    S[:, 0, 1], S[:, 0, 2], S[:, 1, 0], S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = -p[:, 2], p[:, 1], p[:, 2], -p[:, 0], -p[:, 1], p[:, 0]
    J = np.concatenate([R @ S, np.broadcast_to(-R, (len(inl), 3, 3))], axis=2)
    r0 = _residuals(T, p, q)
    rn = np.sqrt(np.einsum("ni,nij,nj->n", r0, M, r0))
    w = irls_weight_fd(loss, rn, scale) if len(inl) else np.zeros(0)
    H = np.einsum("n,nia,nij,njb->ab", g * w, J, M, J)
    b = np.einsum("n,nia,nij,nj->a", g * w, J, M, r0)
    return {"H": H, "b": b, "error": float((g * rho(loss, rn, scale)).sum()), "inlier": len(inl), "w": w, "index": inl}


def error_f64(case, factor, loss, scale, T_trial):
    """K12 at a trial pose (registration.hpp:678-777, what an LM / dog-leg trial step evaluates): correspondences and inlier gate
    stay those of the linearisation, the cost is the cost AT the trial pose — GICP's M is (plane(Ct) + R plane(Cs) R^T)^-1 with the
    trial pose's R."""
    trial = case.with_pose(T_trial)
    _, _, _, _, _, g = _geometry(trial, factor)
    return float((g * rho(loss, residual_norms(trial, factor), scale)).sum())


# ---- comparison per 3x3 block
BLOCKS = {"rot": (slice(0, 3), slice(0, 3)), "trans": (slice(3, 6), slice(3, 6)), "coupling": (slice(0, 3), slice(3, 6))}
HALVES = {"rot": slice(0, 3), "trans": slice(3, 6)}


def relative(diff, size):
    # a block that is exactly zero in float64 (every correspondence rejected, every TUKEY weight zero) has to be exactly zero
    return float(diff / size) if size > 0.0 else (0.0 if diff == 0.0 else np.inf)


def distances(got_H, got_b, got_error, ref, f64_ref=None):
    """max |got - ref| of every 3x3 block of H (rotation, translation, coupling) and of each half of b, each relative to the
    FLOAT64 maximum of that block / half; |error| relative. ref: a dict with H, b, error (the float64 model, or the oracle's
    result with the float64 model as f64_ref: the sizes always come from float64)."""
    got_H, got_b = np.asarray(got_H, np.float64), np.asarray(got_b, np.float64)
    f64_ref = ref if f64_ref is None else f64_ref
    out = {}
    for k, (r, c) in BLOCKS.items():
        out["H_" + k] = relative(np.abs(got_H[r, c] - ref["H"][r, c]).max(), np.abs(f64_ref["H"][r, c]).max())
    for k, s in HALVES.items():
        out["b_" + k] = relative(np.abs(got_b[s] - ref["b"][s]).max(), np.abs(f64_ref["b"][s]).max())
    out["error"] = relative(abs(got_error - ref["error"]), abs(f64_ref["error"]))
    return out
