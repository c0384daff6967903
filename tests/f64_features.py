"""A float64 model of the features stage (K5 - K8: neighbourhood covariance, M-estimated covariance, normalize_covariance,
update_covariance_plane, normals), written FROM THE MATHEMATICS, and the input families the stage is held to it on. A plain helper
module shared by tests/test_features_f64_cpu.py (the oracle, no GPU) and tests/test_gpu_features_f64.py (the kernels).

Kernels and oracle were both written from one reading of covariance.hpp and eigen_utils.hpp, so "GPU == oracle" alone could hide an
error both share (tests/f64_factors.py says the same of the factors). Nothing here restates eigen_utils.hpp: no analytic cubic, no
adjugate, no sum of outer products minus the outer product of the mean.

    covariance      C = sum (p - m)(p - m)^T / k over the valid (idx >= 0) neighbours, m their mean; I when fewer than 4 are valid
    eigen           numpy.linalg.eigh of the float64 image of the float32 matrix, eigenvalues ascending
    normal          the eigenvector of lambda0, up to sign
    plane           I - (1 - 1e-3) n n^T: defined whenever lambda0 is separated, even with lambda1 == lambda2
    normalised      V diag(clamp(l0 / l2, 1e-3, 1), clamp(l1 / l2, 1e-3, 1), 1) V^T; I when l2 (of 1e3 C) is below FLT_MIN
    M-estimate      robust_covariance(): see its docstring for what the reference feeds to the loss and what enters the median

The float32 implementations (the reference's arithmetic, which oracle and kernels reproduce on purpose) lose accuracy with the
conditioning of the input, so every row gets the bound its own conditioning allows:

    error_row <= factor * K[quantity] * eps32 * kappa_row

    kappa of an eigenvector quantity = (lambda_max / min gap of the eigenvalue pairs the quantity depends on)^2, at least 1
        normal                          the pair (l0, l1)
        eigenvector k                   the pairs (lk, every other)
        plane / normalised covariance   all pairs (the float32 product V diag V^T needs V orthogonal, i.e. all three vectors)
    kappa of an eigenvalue = lambda_max / min gap, the first power (error relative to the largest |eigenvalue|)
    kappa of a covariance  = max |p|^2 / max |C64|  (C = E[pp^T] - mm^T in float32: absolute error ~ eps32 max |p|^2)
    kappa of an M-estimate = kappa of the covariance * lambda_max / lambda_min of the plain covariance (the Mahalanobis distances
        go through its inverse), when the inverse is taken; kappa of the covariance when it is not (determinant below the cut)

K[quantity] is MEASURED: the worst error / (eps32 * kappa) of the CPU oracle over all quantitative families
(tests/test_features_f64_cpu.py prints it and holds the oracle to 2 K; the kernels are held to 4 K against float64 and to 4 * 2 K
against the oracle, since device and oracle may each be that far out, in opposite directions). The table is ORACLE_K below.
"""
import numpy as np

import f64_factors as f64f

EPS32 = float(np.finfo(np.float32).eps)
FLT_MIN = float(np.finfo(np.float32).tiny)
PLANE_WEIGHT = 1e-3        # covariance.hpp:71
CLAMP_LO = 1e-3            # covariance.hpp:88-89
DET_CUT = 1e-6             # eigen_utils.hpp:403-423: inverse() returns Zero below it
DET_ABOVE, DET_BELOW = 4e-6, 2.5e-7   # determinants handed to inverse() stay outside (DET_BELOW, DET_ABOVE)
THRESHOLD_MARGIN = 1e-3    # Mahalanobis distances stay this far (relative) from the HUBER / TUKEY threshold
WEIGHT_ONE_BELOW = 1e-8    # robust.hpp:56-63: compute_weight returns 1 for a residual <= 1e-8
ROBUST_LOSSES = ("HUBER", "TUKEY", "CAUCHY", "GEMAN_MCCLURE")

# Worst error / (eps32 * kappa) of the CPU oracle against this model over the quantitative families, measured by
# tests/test_features_f64_cpu.py::test_oracle_constants (x86-64, glibc libm) and rounded up to two digits.
ORACLE_K = {
    "eigenvalue": 4.2,     # kappa = lambda_max / min gap (first power)
    "eigenvector": 2.8,
    "normal": 1.5,
    "plane": 5.5,
    "normalized": 3.4,
    "covariance": 5.4,     # absolute: K eps32 max |p|^2
    "robust": 1.3,
    "inverse": 1.7,        # relative to max |C^-1|, kappa = lambda_max / lambda_min
}
# test hooks: tests/test_features_f64_cpu.py sets one of these to see the comparison fail (and resets it)
MUTATION = None   # "plane_weight" | "normal_is_v1" | "median_valid_only" | "swap_loss"


# ---------------------------------------------------------------------------------------------------------------- the model
def cov3(covs16):
    return f64f.cov3(covs16)


def cov16(C):
    return f64f.cov16(C)


def covariance(pts, idx):
    """(n, 3, 3) float64: centred second moment of each row's valid neighbours, identity with fewer than 4."""
    P = np.asarray(pts, np.float32)[:, :3].astype(np.float64)
    idx = np.asarray(idx)
    out = np.empty((len(idx), 3, 3))
    for i, row in enumerate(idx):
        q = P[row[row >= 0]]
        if len(q) < 4:
            out[i] = np.eye(3)
            continue
        d = q - q.mean(axis=0)
        out[i] = d.T @ d / len(q)
    return out


def eigh(C):
    """Ascending eigenvalues (n, 3) and eigenvectors in columns (n, 3, 3) of float64 symmetric matrices."""
    return np.linalg.eigh(np.asarray(C, np.float64))


def normal(C):
    lam, V = eigh(C)
    return V[..., :, 1] if MUTATION == "normal_is_v1" else V[..., :, 0]


def plane_covariance(C):
    n = normal(C)
    w = 2e-3 if MUTATION == "plane_weight" else PLANE_WEIGHT
    return np.eye(3) - (1.0 - w) * np.einsum("...i,...j->...ij", n, n)


def normalized_covariance(C):
    C = np.asarray(C, np.float64)
    lam, V = eigh(C)
    out = np.empty_like(C)
    for i in range(len(C)):
        l2 = lam[i, 2]
        if 1e3 * l2 < FLT_MIN:
            out[i] = np.eye(3)
            continue
        d = np.array([np.clip(lam[i, 0] / l2, CLAMP_LO, 1.0), np.clip(lam[i, 1] / l2, CLAMP_LO, 1.0), 1.0])
        out[i] = (V[i] * d) @ V[i].T
    return out


def _weighted(P, w):
    m = (w[:, None] * P).sum(axis=0) / w.sum()
    d = P - m
    return m, (w[:, None] * d).T @ d / w.sum()


def robust_covariance(pts, idx, loss, mad_scale, min_scale, max_iterations, trace=None):
    """covariance.hpp:182-222, as mathematics. Per row, with w = 1 at the start:

        m, C   = weighted mean and covariance of the valid neighbours (identity, and the end, with fewer than 4 of them or a total
                 weight below FLT_EPSILON)
        d_j    = (p_j - m)^T C^-1 (p_j - m), the SQUARED Mahalanobis distance, for the valid slots. C^-1 is numpy.linalg.inv;
                 the reference's inverse() answers Zero for |det C| < 1e-6 (every d_j = 0 then), which is a branch of the
                 specification, not arithmetic, and is modelled as such: the families keep determinants away from the cut
        median = the median of d over ALL k slots of the row: a padded slot (idx < 0) keeps its initial distance 0 and is part of
                 it (dist_squared is filled with 0 and only valid slots are written, covariance.hpp:188, 197-203). That is the
                 specification
        scale  = max(mad_scale * median, min_scale)
        w_j    = rho'(r) / r at r = d_j, s = scale: the reference hands the SQUARED distance to compute_weight as the residual
                 (covariance.hpp:212) and the scale is in the same units. rho' is f64_factors.irls_weight_fd's central difference
                 of rho, not a closed form; w = 1 where d_j <= 1e-8 (robust.hpp: compute_weight's first line)

    repeated max_iterations times. trace (a list) receives per row what the branch-safety checks need: (det, d / scale) per round."""
    P = np.asarray(pts, np.float32)[:, :3].astype(np.float64)
    idx = np.asarray(idx)
    use = loss
    if MUTATION == "swap_loss":
        use = {"HUBER": "CAUCHY", "CAUCHY": "HUBER", "TUKEY": "GEMAN_MCCLURE", "GEMAN_MCCLURE": "TUKEY"}[loss]
    out = np.empty((len(idx), 3, 3))
    for i, row in enumerate(idx):
        valid = row >= 0
        rounds = []
        if trace is not None:
            trace.append(rounds)
        if valid.sum() < 4:
            out[i] = np.eye(3)
            continue
        q = P[row[valid]]
        m, C = _weighted(q, np.ones(len(q)))
        for _ in range(max_iterations):
            det = np.linalg.det(C)
            Ci = np.linalg.inv(C) if abs(det) >= DET_CUT else np.zeros((3, 3))
            d = np.zeros(len(row))
            diff = q - m
            d[valid] = np.einsum("ni,ij,nj->n", diff, Ci, diff)
            med = np.median(d[valid]) if MUTATION == "median_valid_only" else np.median(d)
            scale = max(mad_scale * med, min_scale)
            safe = np.maximum(d, 1e-300)
            w = np.where(d <= WEIGHT_ONE_BELOW, 1.0, f64f.irls_weight_fd(use, safe, scale))
            rounds.append((det, d[valid] / scale))
            if w[valid].sum() < EPS32:
                C = np.eye(3)
                break
            m, C = _weighted(q, w[valid])
        out[i] = C
    return out


# ---------------------------------------------------------------------------------------------------------------- conditioning
def _gaps(lam):
    return lam[..., 1] - lam[..., 0], lam[..., 2] - lam[..., 1], lam[..., 2] - lam[..., 0]


def _kappa(lmax, gap):
    with np.errstate(divide="ignore", invalid="ignore"):
        k = (lmax / gap) ** 2
    return np.where(gap > 0, np.maximum(k, 1.0), np.inf)


def kappas(C):
    """Per row: dict of kappa for 'normal', 'vec0', 'vec1', 'vec2', 'all' from the float64 spectrum of C."""
    lam, _ = eigh(C)
    lmax = np.abs(lam).max(axis=-1)
    g01, g12, _ = _gaps(lam)
    return {"normal": _kappa(lmax, g01), "vec0": _kappa(lmax, g01), "vec1": _kappa(lmax, np.minimum(g01, g12)),
            "vec2": _kappa(lmax, g12), "all": _kappa(lmax, np.minimum(g01, g12))}


def kappa_cov(pts, idx, C64):
    """max(max |p|^2, max |C64|) / max |C64| per row, and the numerator: error <= K eps32 kappa max |C64| is the absolute bound
    K eps32 max |p|^2 (a row whose covariance is exactly zero, identical points, has it too)."""
    P = np.asarray(pts, np.float32)[:, :3].astype(np.float64)
    idx = np.asarray(idx)
    size = np.abs(C64).max(axis=(1, 2))
    p2 = np.array([np.abs(P[r[r >= 0]]).max() ** 2 if (r >= 0).any() else 1.0 for r in idx])
    p2 = np.maximum(p2, size)
    with np.errstate(divide="ignore"):
        return np.where(size > 0, p2 / size, np.inf), p2


# ---------------------------------------------------------------------------------------------------------------- errors per row
def err_eigenvalues(vals, C):
    lam, _ = eigh(C)
    lmax = np.abs(lam).max(axis=-1)
    e = np.abs(np.asarray(vals, np.float64) - lam).max(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(lmax > 0, e / lmax, np.where(e == 0, 0.0, np.inf))


def err_direction(v, v64):
    """max |v - s v64| with s the sign that aligns them: linear in the angle, and it sees a wrong length too."""
    v, v64 = np.asarray(v, np.float64), np.asarray(v64, np.float64)
    s = np.sign(np.einsum("...i,...i->...", v, v64))
    s = np.where(s == 0, 1.0, s)
    return np.abs(v - s[..., None] * v64).max(axis=-1)


def err_matrix(M, M64):
    return np.abs(np.asarray(M, np.float64) - M64).max(axis=(-2, -1))


def ratio(err, kappa):
    """error / (eps32 * kappa) per row; a row whose kappa is infinite asks nothing (ratio 0) and must not be in a quantitative
    family (the families assert that)."""
    return np.where(np.isfinite(kappa), err / (EPS32 * np.where(np.isfinite(kappa), kappa, 1.0)), 0.0)


# ---------------------------------------------------------------------------------------------------------------- families
def rotations(rs, n):
    return f64f.random_rotations(rs, n)


def spectrum_matrices(rs, lam, n):
    """n float32 covariance rows (n, 16) V diag(lam) V^T with random rotations V, exactly symmetric."""
    V = rotations(rs, n)
    C = np.einsum("nik,k,njk->nij", V, np.asarray(lam, np.float64), V)
    C = 0.5 * (C + C.transpose(0, 2, 1))
    return cov16(C.astype(np.float32))


PLANAR_RATIOS = (0.5, 0.1, 1e-2, 1e-3, 1e-5, 0.0)
IN_PLANE_GAPS = (1.0, 0.3, 0.1, 0.03)
MIN_QUANTITATIVE_GAP = 0.03 * 0.9   # relative to lambda_max: the narrowest family, (0.01, 1, 1.03), has 0.03 / 1.03


def matrix_families(n=300, seed=20250117):
    """name -> (class, (n, 16) float32 rows). class: 'quantitative' (everything bounded), 'normal_only' (normal and eigenvalues
    bounded; lambda1 ~ lambda2), 'degenerate' (invariants only)."""
    rs = np.random.RandomState(seed)
    fam = {"generic_1_2_3": ("quantitative", spectrum_matrices(rs, (1, 2, 3), n))}
    for scale, tag in ((1.0, "planar"), (1e-4, "lidar"), (1e-12, "tiny")):
        for r in PLANAR_RATIOS:
            fam[f"{tag}_{r:g}"] = ("quantitative", spectrum_matrices(rs, np.array([r, 1.0, 2.0]) * scale, n))
    for g in IN_PLANE_GAPS:
        fam[f"gap_{g:g}"] = ("quantitative", spectrum_matrices(rs, (0.01, 1.0, 1.0 + g), n))
    fam["spread_1_2_100"] = ("quantitative", spectrum_matrices(rs, (1, 2, 100), n))
    # lambda1 == lambda2: I - 0.99 n n^T, whose in-plane eigenvectors are anybody's choice
    fam["disc_equal"] = ("normal_only", spectrum_matrices(rs, (0.01, 1.0, 1.0), n))
    fam["disc_gap_1e-3"] = ("normal_only", spectrum_matrices(rs, (0.01, 1.0, 1.001), n))
    fam["line"] = ("degenerate", spectrum_matrices(rs, (0.0, 0.0, 1.0), n))
    fam["isotropic"] = ("degenerate", cov16(np.broadcast_to(np.eye(3, dtype=np.float32), (n, 3, 3)) *
                                            rs.uniform(0.5, 2.0, (n, 1, 1)).astype(np.float32)))
    fam["near_isotropic"] = ("degenerate", spectrum_matrices(rs, (1.0, 1.0001, 1.0002), n))
    fam["zero"] = ("degenerate", np.zeros((n, 16), np.float32))
    fam["below_flt_min"] = ("degenerate", spectrum_matrices(rs, np.array([1.0, 2.0, 3.0]) * 1e-39, n))
    # the solver's |disc| <= FLT_EPSILON branch, entered with exact coefficients: diagonal matrices with a double eigenvalue
    d = np.zeros((n, 3, 3), np.float32)
    d[:, 0, 0], d[:, 1, 1], d[:, 2, 2] = 1.0, 1.0, 0.25
    d[n // 2:, 2, 2] = 4.0
    fam["diag_double"] = ("degenerate", cov16(d))
    # its |p| < FLT_EPSILON branch (taken only when |disc| is above FLT_EPSILON). For a SYMMETRIC matrix scaled to max |entry| = 1,
    # p = -sum (li - lj)^2 / 6 and disc = -prod (li - lj)^2: |p| < eps32 forces |disc| < eps32^3, so no covariance reaches it. The
    # solver reads both triangles, though, and a cyclic permutation matrix (times a scale) has p = 0 exactly and q = -1: these rows
    # enter the branch. They are not covariances; only the invariants (finite, unit columns, device == oracle) are asked of them
    c = np.zeros((n, 3, 3), np.float32)
    c[:, 0, 1] = c[:, 1, 2] = c[:, 2, 0] = 1.0
    c[1::2] = c[1::2].transpose(0, 2, 1)
    fam["p_branch_cyclic"] = ("degenerate", cov16(c * (2.0 ** rs.randint(-20, 20, (n, 1, 1))).astype(np.float32)))
    for name, (cls, rows) in fam.items():
        if cls == "quantitative":
            lam, _ = eigh(cov3(rows))
            g01, g12, _ = _gaps(lam)
            # (1, 2, 100) is the one family below that: its smallest gap is 1 % of lambda_max, kappa = 1e4, and it is what shows
            # that the bound scales with kappa as claimed
            floor = 0.009 if name == "spread_1_2_100" else MIN_QUANTITATIVE_GAP
            assert (np.minimum(g01, g12) >= floor * np.abs(lam).max(axis=1)).all(), name
    return fam


def solver_branches(C):
    """Which branch of the analytic solver the depressed cubic of each row belongs to, evaluated in float64 from the characteristic
    polynomial of the matrix scaled to max |entry| = 1 (x^3 + c2 x^2 + c1 x + c0, c2 = -trace, c1 = the sum of the principal 2x2
    minors, c0 = -det; p = c1 - c2^2 / 3, q = 2 c2^3 / 27 - c2 c1 / 3 + c0, disc = 4 p^3 + 27 q^2): 'disc' (|disc| <= FLT_EPSILON),
    'p' (|p| < FLT_EPSILON with |disc| above), 'trig'. Only used to show that a family built for a branch enters it."""
    C = np.asarray(C, np.float64)
    mx = np.abs(C).max(axis=(1, 2))
    S = C / np.where(mx > 0, mx, 1.0)[:, None, None]
    c2 = -np.trace(S, axis1=1, axis2=2)
    c1 = sum(S[:, i, i] * S[:, j, j] - S[:, i, j] * S[:, j, i] for i, j in ((0, 1), (0, 2), (1, 2)))
    c0 = -np.linalg.det(S)
    p = c1 - c2 * c2 / 3.0
    q = 2.0 * c2 ** 3 / 27.0 - c2 * c1 / 3.0 + c0
    disc = 4.0 * p ** 3 + 27.0 * q * q
    return np.where(np.abs(disc) <= EPS32, "disc", np.where(np.abs(p) < EPS32, "p", "trig"))


def unit_shape(rs, k):
    """k points with mean exactly ~0 and second moment ~I (whitened Gaussian draw): Z diag(sqrt(lam)) V^T has spectrum lam."""
    z = rs.normal(size=(k, 3))
    z -= z.mean(axis=0)
    L = np.linalg.cholesky(z.T @ z / k)
    return z @ np.linalg.inv(L).T


class Neighbourhoods:
    """groups x k points; every point of a group lists the whole group (each member in its own rotation of the order, so that the
    float32 sums are formed in k different orders). pts (groups * k, 4) float32, idx (groups * k, k) int32."""

    def __init__(self, pts, idx, k):
        self.pts, self.idx, self.k = pts, idx, k


def neighbourhoods(rs, lam, groups, k, centre=(0.0, 0.0, 0.0), centre_spread=0.0):
    lam = np.asarray(lam, np.float64)
    V = rotations(rs, groups)
    pts = np.ones((groups * k, 4), np.float32)
    idx = np.empty((groups * k, k), np.int32)
    for g in range(groups):
        z = unit_shape(rs, k) * np.sqrt(lam)
        c = np.asarray(centre) + rs.uniform(-centre_spread, centre_spread, 3)
        pts[g * k:(g + 1) * k, :3] = z @ V[g].T + c
        base = np.arange(k) + g * k
        for j in range(k):
            idx[g * k + j] = np.roll(base, -j)
    return Neighbourhoods(pts, idx, k)


def neighbourhood_families(seed=20250118, groups=15, k=20):
    """name -> (class, Neighbourhoods), spectra as in matrix_families (the lengths are standard deviations of metres)."""
    rs = np.random.RandomState(seed)
    fam = {"generic_1_2_3": ("quantitative", neighbourhoods(rs, (1, 2, 3), groups, k))}
    for r in (0.1, 1e-2, 1e-3):
        fam[f"planar_{r:g}"] = ("quantitative", neighbourhoods(rs, (r, 1.0, 2.0), groups, k))
        fam[f"lidar_{r:g}"] = ("quantitative", neighbourhoods(rs, np.array([r, 1.0, 2.0]) * 1e-4, groups, k))
    for g in (1.0, 0.1):
        fam[f"gap_{g:g}"] = ("quantitative", neighbourhoods(rs, (0.01, 1.0, 1.0 + g), groups, k))
    return fam


def patch_families(seed=20250119, groups=10, k=20):
    """The same 10 cm and 50 cm patches (standard deviations (0.01, 0.5, 1) x size) centred 0, 1, 5, 20 and 100 m out."""
    fam = {}
    for size in (0.1, 0.5):
        for dist in (0.0, 1.0, 5.0, 20.0, 100.0):
            rs = np.random.RandomState(seed)  # the same shapes at every distance
            c = np.array([0.6, -0.64, 0.48]) * dist
            fam[f"patch_{size:g}m_at_{dist:g}m"] = neighbourhoods(rs, np.array([1e-4, 0.25, 1.0]) * size * size, groups, k, centre=c)
    return fam


def degenerate_neighbourhoods(k=20):
    """20 identical points, exactly collinear neighbours, a square-lattice patch z = const (lambda1 == lambda2 exactly)."""
    out = {}
    pts = np.ones((k, 4), np.float32)
    pts[:, :3] = (0.3, -1.7, 2.2)
    out["identical"] = Neighbourhoods(pts, np.tile(np.arange(k, dtype=np.int32), (k, 1)), k)
    pts = np.ones((k, 4), np.float32)
    pts[:, :3] = np.arange(k, dtype=np.float32)[:, None] * np.array([0.25, 0.5, -0.125], np.float32)
    out["collinear"] = Neighbourhoods(pts, np.tile(np.arange(k, dtype=np.int32), (k, 1)), k)
    side = 5
    gx, gy = np.meshgrid(np.arange(side), np.arange(side))
    pts = np.ones((side * side, 4), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = gx.ravel() * 0.125, gy.ravel() * 0.125, 1.5
    out["lattice"] = Neighbourhoods(pts, np.tile(np.arange(side * side, dtype=np.int32), (side * side, 1)), side * side)
    return out


def flip_family(seed=20250120, n=600):
    """Covariances with a well-separated normal and points placed at chosen n64.p: the five classes of the flip rule
    (covariance.hpp:54: the normal is negated when n.p > 1). Returns (pts (n, 4), covs (n, 16), t = n64.p (n,), n64 (n, 3))."""
    rs = np.random.RandomState(seed)
    covs = spectrum_matrices(rs, (0.01, 1.0, 2.0), n)
    n64 = normal(cov3(covs))
    targets = np.array([3.0, -3.0, 1.0 + 2e-3, -(1.0 + 2e-3), 1.0 - 2e-3, -(1.0 - 2e-3), 0.4, -0.4, 1.0 + 1e-3 * 1.01, 1.0 - 1e-3 * 1.01])
    t = targets[np.arange(n) % len(targets)]
    inplane = rs.normal(size=(n, 3)) * 2.0
    inplane -= np.einsum("ni,ni->n", inplane, n64)[:, None] * n64
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = t[:, None] * n64 + inplane
    t32 = np.einsum("ni,ni->n", pts[:, :3].astype(np.float64), n64)
    assert (np.abs(np.abs(t32) - 1.0) >= 1e-3).all()
    return pts, covs, t32, n64


# ---------------------------------------------------------------------------------------------------------------- robust inputs
def robust_family(seed, groups, k, lam, mad_scale, min_scale, iterations, pad=None, centre_spread=0.5):
    """Neighbourhoods on which NO float32 implementation can fall on the other side of a branch of the M-estimate, for every loss
    and every round up to `iterations`: candidates are drawn and kept only when, in the float64 model,
      * every determinant handed to inverse() is >= 4e-6 or <= 2.5e-7 (the cut is 1e-6);
      * with the inverse taken, every d / scale is at least 1e-3 (relative) from 1 (the HUBER and TUKEY threshold) and at least a
        quarter of the row's valid neighbours lie on each side.
    pad: positions (within a row) set to -1."""
    rs = np.random.RandomState(seed)
    kept_pts, kept_idx = [], []
    tries = 0
    while len(kept_pts) < groups:
        tries += 1
        assert tries < 50 * groups, "robust_family: cannot find enough branch-safe neighbourhoods"
        nb = neighbourhoods(rs, lam, 1, k, centre_spread=centre_spread)
        idx = nb.idx.copy()
        if pad:
            idx[:, list(pad)] = -1
        if branch_safe(nb.pts, idx, mad_scale, min_scale, iterations):
            kept_pts.append(nb.pts)
            kept_idx.append(idx + len(kept_idx) * k * (idx >= 0))
    return Neighbourhoods(np.concatenate(kept_pts), np.concatenate(kept_idx).astype(np.int32), k)


def branch_safe(pts, idx, mad_scale, min_scale, iterations, losses=ROBUST_LOSSES):
    for loss in losses:
        trace = []
        robust_covariance(pts, idx, loss, mad_scale, min_scale, iterations, trace=trace)
        for rounds in trace:
            for det, x in rounds:
                if DET_BELOW < abs(det) < DET_ABOVE:
                    return False
                if abs(det) >= DET_CUT:
                    if (np.abs(x - 1.0) < THRESHOLD_MARGIN).any():
                        return False
                    if (x < 1.0).mean() < 0.25 or (x > 1.0).mean() < 0.25:
                        return False
    return True


# ---------------------------------------------------------------------------------------------------------------- the comparison
# An implementation (tests/test_features_f64_cpu.py: the oracle; tests/test_gpu_features_f64.py: the device entries) offers
#   eigen3(rows16) -> (vals (n, 3), vecs (n, 3, 3) columns)      inverse3(rows16) -> (n, 3, 3)
#   cov(pts, idx) -> (n, 16)      normals_knn(pts, idx) -> (n, 4)      normals_cov(pts, covs16) -> (n, 4)
#   plane(covs16) -> (n, 16)      normalize(covs16) -> (n, 16)         robust(pts, idx, loss, mad, min_scale, iterations) -> (n, 16)
# collect() runs every family through it, score() turns the outputs into error / (eps32 * kappa) per (quantity, family) against
# float64 (or against another implementation's outputs) and asserts the invariants on the way.
# mad_scale is not 1: with an odd k the median IS one of the distances, and d / scale would sit on the threshold exactly
ROBUST_SETTINGS = {"mad_scale": 1.25, "min_scale": 0.5}
# degenerate inputs. Next to a DOUBLE root acosf's argument is next to 1 and d(acos x) = dx / sqrt(1 - x^2) with dx a few eps32:
# an eigenvalue is good to about sqrt(eps32) of the largest, 4 sqrt(eps32) is the bound
DOUBLE_ROOT_EIGENVALUE_BOUND = 4.0 * np.sqrt(EPS32)
# |disc| <= FLT_EPSILON next to a TRIPLE root: the eigenvalues are -c2 / 3 + {2u, -u, -u}, u = cbrt(q / 2), and q, a sum of terms
# of size 2, 3 and 1, is rounding noise of up to ~16 eps32: u <= cbrt(8 eps32), an eigenvalue is off by up to 2 u = 4 cbrt(eps32)
TRIPLE_ROOT_EIGENVALUE_BOUND = 4.0 * np.cbrt(EPS32)
TRIPLE_ROOT_FAMILIES = ("isotropic", "near_isotropic")
EXACT_IDENTITY_FAMILIES = ("zero", "below_flt_min")    # max |entry| < FLT_MIN: eigenvalues 0, eigenvectors I (eigen_utils.hpp:455-460)
NOT_A_COVARIANCE = ("p_branch_cyclic",)


_cache = {}


def cached(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def robust_families():
    """name -> (Neighbourhoods, iterations its branch safety was established for)."""
    def make():
        lam = (0.05, 0.3, 1.0)   # determinant 0.015, lambda_max / lambda_min = 20
        return {
            "blob_k20": (robust_family(1, 8, 20, lam, iterations=3, **ROBUST_SETTINGS), 3),
            "blob_k5": (robust_family(2, 8, 5, lam, iterations=3, **ROBUST_SETTINGS), 3),
            "blob_k20_pad_mid": (robust_family(3, 8, 20, lam, iterations=3, pad=(0, 7, 8), **ROBUST_SETTINGS), 3),
            # LiDAR scale: determinant 1.5e-14, inverse() answers Zero, every distance is 0, every weight 1
            "lidar_k20": (robust_family(4, 8, 20, np.array(lam) * 1e-4, iterations=3, **ROBUST_SETTINGS), 3),
        }
    return cached("robust", make)


class OracleFeatures:
    def __init__(self, orc):
        self.orc = orc

    def eigen3(self, rows):
        C = cov3(rows).astype(np.float32)
        vals, vecs = np.empty((len(C), 3), np.float32), np.empty((len(C), 3, 3), np.float32)
        for i in range(len(C)):
            vals[i], vecs[i] = self.orc.eigen3(C[i])
        return vals, vecs

    def inverse3(self, rows):
        C = cov3(rows).astype(np.float32)
        return np.stack([self.orc.inverse3(c) for c in C])

    def cov(self, pts, idx):
        return self.orc.cov_estimate(pts, idx)

    def normals_knn(self, pts, idx):
        return self.orc.normals_from_knn(pts, idx)

    def normals_cov(self, pts, covs):
        return self.orc.normals_from_cov(pts, covs)

    def plane(self, rows):
        return self.orc.update_covariance_plane(rows)

    def normalize(self, rows):
        return self.orc.cov_normalize(rows)

    def robust(self, pts, idx, loss, mad_scale, min_scale, iterations):
        return self.orc.cov_estimate_robust(pts, idx, loss, mad_scale, min_scale, iterations)


def collect(impl):
    out = {}
    for name, (cls, rows) in cached("matrix", matrix_families).items():
        vals, vecs = impl.eigen3(rows)
        out["eigen", name] = (np.asarray(vals), np.asarray(vecs))
        out["plane", name] = np.asarray(impl.plane(rows))
        out["normalized", name] = np.asarray(impl.normalize(rows))
        out["inverse", name] = np.asarray(impl.inverse3(rows))
        # the normal of the same matrix for a point at the origin (n.p = 0: never flipped)
        out["normal_of", name] = np.asarray(impl.normals_cov(np.tile(np.float32([[0, 0, 0, 1]]), (len(rows), 1)), rows))
    for name, (cls, nb) in cached("nbhd", neighbourhood_families).items():
        c = np.asarray(impl.cov(nb.pts, nb.idx))
        out["cov", name] = c
        out["normals_knn", name] = np.asarray(impl.normals_knn(nb.pts, nb.idx))
        out["normals_cov", name] = np.asarray(impl.normals_cov(nb.pts, c))
    for name, nb in cached("patch", patch_families).items():
        out["cov", name] = np.asarray(impl.cov(nb.pts, nb.idx))
    for name, nb in cached("degnb", degenerate_neighbourhoods).items():
        c = np.asarray(impl.cov(nb.pts, nb.idx))
        out["cov", name] = c
        out["normals_knn", name] = np.asarray(impl.normals_knn(nb.pts, nb.idx))
        out["plane_of_cov", name] = np.asarray(impl.plane(c))
        out["normalized_of_cov", name] = np.asarray(impl.normalize(c))
    pts, covs, _, _ = cached("flip", flip_family)
    out["normals_cov", "flip"] = np.asarray(impl.normals_cov(pts, covs))
    for name, (nb, its) in robust_families().items():
        for loss in ROBUST_LOSSES:
            for it in (1, 3):
                out["robust", name, loss, it] = np.asarray(impl.robust(nb.pts, nb.idx, loss, ROBUST_SETTINGS["mad_scale"],
                                                                       ROBUST_SETTINGS["min_scale"], it))
        out["cov", "robust_" + name] = np.asarray(impl.cov(nb.pts, nb.idx))
    return out


def _finite(tag, *arrays):
    for a in arrays:
        assert np.isfinite(a).all(), f"{tag}: a non-finite output"


def _symmetric16(tag, rows, symmetrised=True):
    """covariance.hpp symmetrises (ensure_symmetric) the plain and the M-estimated covariance: those are bitwise symmetric. The
    plane and the normalised covariance are products V diag V^T nobody symmetrises: only their padding is checked."""
    M = np.asarray(rows).reshape(-1, 4, 4)
    if symmetrised:
        assert np.array_equal(M[:, :3, :3], M[:, :3, :3].transpose(0, 2, 1)), f"{tag}: not bitwise symmetric"
    assert not M[:, 3, :].any() and not M[:, :, 3].any(), f"{tag}: the padding row / column of a stored covariance must be zero"


def _references():
    """Everything float64 the scores need, computed once."""
    def make():
        ref = {}
        for name, (cls, rows) in cached("matrix", matrix_families).items():
            C = cov3(rows)
            lam, V = eigh(C)
            ref["matrix", name] = {"C": C, "lam": lam, "V": V, "kappa": kappas(C), "plane": plane_covariance(C), "n": normal(C),
                                   "normalized": normalized_covariance(C), "det": np.linalg.det(C)}
        for group in ("nbhd", "patch", "degnb"):
            fams = cached(group, {"nbhd": neighbourhood_families, "patch": patch_families, "degnb": degenerate_neighbourhoods}[group])
            for name, nb in fams.items():
                nb = nb[1] if isinstance(nb, tuple) else nb
                C = covariance(nb.pts, nb.idx)
                kc, p2 = kappa_cov(nb.pts, nb.idx, C)
                ref["cov", name] = {"C": C, "kappa": kc, "p2": p2, "kvec": kappas(C), "normal": normal(C)}
        for name, (nb, its) in robust_families().items():
            C = covariance(nb.pts, nb.idx)
            lam, _ = eigh(C)
            kc, p2 = kappa_cov(nb.pts, nb.idx, C)
            inverted = np.abs(np.linalg.det(C)) >= DET_CUT
            ref["cov", "robust_" + name] = {"C": C, "kappa": kc, "p2": p2}
            for loss in ROBUST_LOSSES:
                for it in (1, 3):
                    ref["robust", name, loss, it] = {
                        "C": robust_covariance(nb.pts, nb.idx, loss, ROBUST_SETTINGS["mad_scale"], ROBUST_SETTINGS["min_scale"], it),
                        "kappa": np.where(inverted, kc * lam[:, 2] / lam[:, 0], kc), "inverted": inverted}
        return ref
    if MUTATION is not None:   # a mutated model is never cached
        return make()
    return cached("ref", make)


def score(out, other=None):
    """{(quantity, family...): worst error / (eps32 * kappa) over the rows} of `out` against float64, or against `other` (another
    implementation's collect()) with the float64 model still supplying kappa and the sizes. Only families with a quantitative claim
    appear; the invariants of every family are asserted on the way (against float64 only)."""
    ref = _references()
    res = {}
    pair = other is not None

    def put(key, err, kappa):
        assert np.isfinite(kappa).all(), (key, "a quantitative row with infinite kappa")
        res[key] = float(ratio(err, kappa).max())

    for name, (cls, rows) in cached("matrix", matrix_families).items():
        r = ref["matrix", name]
        vals, vecs = out["eigen", name]
        tag = f"eigen3[{name}]"
        _finite(tag, vals, vecs, out["plane", name], out["normalized", name], out["inverse", name])
        if not pair:
            assert (np.diff(vals, axis=1) >= 0).all(), f"{tag}: eigenvalues not ascending"
            assert np.abs(np.linalg.norm(vecs.astype(np.float64), axis=1) - 1.0).max() <= 4 * EPS32, f"{tag}: eigenvector not of unit length"
            # one solver everywhere: the stored normal IS the first eigenvector, bit for bit (csrc/sp_cov_normal.h's promise)
            assert np.array_equal(out["normal_of", name][:, :3], vecs[:, :, 0]) and not out["normal_of", name][:, 3].any(), \
                f"{tag}: the normal of a covariance is not the solver's first eigenvector"
            _symmetric16(f"plane[{name}]", out["plane", name], symmetrised=False)
            _symmetric16(f"normalized[{name}]", out["normalized", name], symmetrised=False)
            if name in EXACT_IDENTITY_FAMILIES:
                assert not vals.any() and np.array_equal(vecs, np.broadcast_to(np.eye(3, dtype=vecs.dtype), vecs.shape)), tag
                if name == "zero":   # (1e3 C of the other family is a normal number again)
                    assert np.array_equal(cov3(out["normalized", name]), np.broadcast_to(np.eye(3), (len(rows), 3, 3))), name
            elif name not in NOT_A_COVARIANCE and cls != "quantitative":
                bound = TRIPLE_ROOT_EIGENVALUE_BOUND if name in TRIPLE_ROOT_FAMILIES else DOUBLE_ROOT_EIGENVALUE_BOUND
                e = err_eigenvalues(vals, r["C"]).max()
                assert e <= bound, f"{tag}: eigenvalue error {e:.2e} of lambda_max above {bound:.2e}"
        lam_o, V_o = (r["lam"], r["V"]) if not pair else other["eigen", name]
        lmax = np.abs(r["lam"]).max(axis=1)
        if cls == "quantitative":
            put(("eigenvalue", name), np.abs(vals - lam_o).max(axis=1) / lmax, np.sqrt(r["kappa"]["all"]))
            for k in range(3):
                put(("eigenvector", name, k), err_direction(vecs[:, :, k], V_o[:, :, k]), r["kappa"][f"vec{k}"])
            put(("plane", name), err_matrix(cov3(out["plane", name]), r["plane"] if not pair else cov3(other["plane", name])), r["kappa"]["all"])
            put(("normalized", name), err_matrix(cov3(out["normalized", name]),
                                                 r["normalized"] if not pair else cov3(other["normalized", name])), r["kappa"]["all"])
        elif cls == "normal_only":
            put(("normal", name), err_direction(vecs[:, :, 0], r["n"] if not pair else V_o[:, :, 0]), r["kappa"]["normal"])
        # inverse(): Zero below the cut, the inverse above it; the families' determinants are nowhere near 1e-6
        inv = out["inverse", name]
        if name not in NOT_A_COVARIANCE:
            det = r["det"]
            assert ((np.abs(det) >= DET_ABOVE) | (np.abs(det) <= DET_BELOW)).all(), f"{name}: a determinant next to the cut"
            above = np.abs(det) >= DET_ABOVE
            assert not inv[~above].any(), f"inverse3[{name}]: Zero expected below the determinant cut"
            if above.any() and cls == "quantitative":
                Ci = np.linalg.inv(r["C"][above]) if not pair else other["inverse", name][above]
                cond = (np.abs(r["lam"]).max(axis=1) / np.abs(r["lam"]).min(axis=1))[above]
                size = np.abs(np.linalg.inv(r["C"][above])).max(axis=(1, 2))
                put(("inverse", name), err_matrix(inv[above], Ci) / size, cond)

    for key in [k for k in out if k[0] == "cov"]:
        name = key[1]
        r = ref["cov", name]
        c = out[key]
        _finite(f"cov[{name}]", c)
        if not pair:
            _symmetric16(f"cov[{name}]", c)
        put(("covariance", name), err_matrix(cov3(c), r["C"] if not pair else cov3(other[key])) / r["p2"], np.ones(len(c)))

    for key in [k for k in out if k[0] in ("normals_knn", "normals_cov") and k[1] != "flip"]:
        name = key[1]
        r = ref["cov", name]
        nrm = out[key]
        _finite(f"{key[0]}[{name}]", nrm)
        assert not nrm[:, 3].any()
        if name in cached("nbhd", neighbourhood_families):
            # the float32 covariance the normal is taken of is itself off by eps32 kappa_cov: both conditionings multiply
            put((key[0], name), err_direction(nrm[:, :3], r["normal"] if not pair else other[key][:, :3]),
                r["kvec"]["normal"] * r["kappa"])
        elif not pair:
            assert np.abs(np.linalg.norm(nrm[:, :3].astype(np.float64), axis=1) - 1.0).max() <= 4 * EPS32, key
    if not pair:
        # identical points: every sum is exact up to the division, the covariance is ~0; a lattice plane z = const: the normal is
        # +-e_z whatever the in-plane vectors do (lambda1 == lambda2 exactly)
        # (coordinates are multiples of 1/8 below 2: every sum is exact, what is left is three roundings of entries of size
        # |x z| <= 0.75, ~3e-7, against in-plane eigenvalues of 0.03: a tilt below 1e-4, far inside 1e-3, and 1 - |nz| ~ 1e-8)
        lat = out["normals_knn", "lattice"]
        assert np.abs(np.abs(lat[:, 2]) - 1.0).max() <= 1e-6 and np.abs(lat[:, :2]).max() <= 1e-3, "lattice plane: normal is not +-e_z"
        for name in cached("degnb", degenerate_neighbourhoods):
            _finite(name, out["plane_of_cov", name], out["normalized_of_cov", name])
            _symmetric16(name, out["plane_of_cov", name], symmetrised=False)
            _symmetric16(name, out["normalized_of_cov", name], symmetrised=False)

    for key in [k for k in out if k[0] == "robust"]:
        _, name, loss, it = key
        r = ref[key]
        c = out[key]
        _finite(str(key), c)
        if not pair:
            _symmetric16(str(key), c)
            if not r["inverted"].any():   # the reference's inverse() answered Zero: the robust estimate IS the plain one
                assert np.array_equal(c, out["cov", "robust_" + name]), f"{key}: must equal the plain covariance bit for bit"
        err = err_matrix(cov3(c), r["C"] if not pair else cov3(other[key]))
        if r["inverted"].all():
            put(("robust", name, loss, it), err / np.abs(r["C"]).max(axis=(1, 2)), r["kappa"])
        else:   # the plain covariance, and its bound
            assert not r["inverted"].any()
            put(("covariance", "robust_" + name, loss, it), err / ref["cov", "robust_" + name]["p2"], np.ones(len(c)))
    return res


def score_flip(nrm, oracle_nrm=None):
    """The flip rule (covariance.hpp:54-64) on flip_family(): asserts, returns nothing."""
    pts, covs, t, n64 = cached("flip", flip_family)
    r = np.asarray(nrm)[:, :3].astype(np.float64)
    p = pts[:, :3].astype(np.float64)
    assert (np.einsum("ni,ni->n", r, p) <= 1.0).all(), "a stored normal has r.p > 1"
    det = np.abs(t) > 1.0 + 1e-3
    assert det.sum() >= len(t) // 4 and (t[det] > 0).any() and (t[det] < 0).any()
    want = -np.sign(t[det])[:, None] * n64[det]
    assert (np.einsum("ni,ni->n", r[det], want) > 0.999).all(), "a determined sign is wrong (asked of 100 % of the rows)"
    inner = np.abs(t) < 1.0
    assert inner.sum() >= len(t) // 4
    if oracle_nrm is not None:
        o = np.asarray(oracle_nrm)[:, :3].astype(np.float64)
        assert (np.einsum("ni,ni->n", r[inner], o[inner]) > 0.999).all(), "|n.p| < 1: the sign is the algorithm's own; device != oracle"
    assert err_direction(r, n64).max() <= 4 * ORACLE_K["normal"] * EPS32 * kappas(cov3(covs))["normal"].max()


def worst(res):
    """{quantity: (worst ratio, its key)} of a score()."""
    out = {}
    for key, v in res.items():
        q = {"normals_knn": "normal", "normals_cov": "normal"}.get(key[0], key[0])
        if q not in out or v > out[q][0]:
            out[q] = (v, key)
    return out
