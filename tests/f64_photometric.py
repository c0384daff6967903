"""float64 model of the photometric term (csrc/photometric.hip), a small float64 aligner, and the generators its tests share.

The model evaluates the formulas of include/sycl_points_amd.h ("photometric (intensity) term") in float64 ON THE float32 INPUTS the
library gets, branch for branch: what it returns is what an exact evaluation of the same inputs would give, so the difference to
the library is the library's rounding alone. Nothing here calls the library.
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
LOSSES = ["NONE", "HUBER", "TUKEY", "CAUCHY", "GEMAN_MCCLURE"]
DET_MIN = 1e-6  # the threshold of the library's symmetric inverse (sp_math.h / sp_linearize.h)


# ------------------------------------------------------------------------------------------------------------ small helpers
def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def random_pose(rng, max_angle_deg=30.0, max_t=5.0):
    """a rotation of up to max_angle_deg about a random axis and a translation of up to max_t per axis"""
    return pose(rotation(rng.normal(size=3), np.deg2rad(rng.uniform(0.2, 1.0) * max_angle_deg)), rng.uniform(-max_t, max_t, 3))


def se3_exp(xi):
    """rotation-first twist [w, v] -> 4x4 (the library's se3_exp)"""
    w, v = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        R, V = np.eye(3) + K, np.eye(3) + 0.5 * K
    else:
        A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / th**2, (th - np.sin(th)) / th**3
        R, V = np.eye(3) + A * K + B * (K @ K), np.eye(3) + B * K + Cc * (K @ K)
    return pose(R, V @ v)


def skew(s):
    z = np.zeros(len(s))
    return np.stack([np.stack([z, -s[:, 2], s[:, 1]], -1), np.stack([s[:, 2], z, -s[:, 0]], -1), np.stack([-s[:, 1], s[:, 0], z], -1)], 1)


def knn_self(points, k):
    """k nearest neighbours of every point in its own cloud (itself included), cKDTree on float64 copies: int32 (n, k), -1 padded"""
    from scipy.spatial import cKDTree

    P = np.asarray(points, np.float64)[:, :3]
    kk = min(k, len(P))
    _, idx = cKDTree(P).query(P, k=kk)
    idx = np.asarray(idx).reshape(len(P), kk)
    out = np.full((len(P), k), -1, np.int32)
    out[:, :kk] = idx
    return out


def nearest(queries, targets):
    """nearest target of every query: (int32 index, float32 squared distance formed as the library's dist2 would be on float32)"""
    from scipy.spatial import cKDTree

    _, idx = cKDTree(np.asarray(targets, np.float64)[:, :3]).query(np.asarray(queries, np.float64)[:, :3], k=1)
    d = (np.asarray(queries, np.float32)[:, :3] - np.asarray(targets, np.float32)[idx, :3]).astype(np.float64)
    return idx.astype(np.int32), (d * d).sum(1).astype(np.float32)


def transform32(T, pts):
    """T applied to (n, 4) float32 points in float64, rounded once"""
    out = np.ones((len(pts), 4), np.float32)
    out[:, :3] = (np.asarray(pts, np.float64)[:, :3] @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------------------ generators
def plane_intensity(x, y):
    return 0.5 + 0.25 * np.sin(2 * np.pi * x / 4 + 0.3) + 0.25 * np.sin(2 * np.pi * y / 5 + 1.1) * np.cos(2 * np.pi * x / 7)


def plane_intensity_gradient(x, y):
    gx = (0.25 * (2 * np.pi / 4) * np.cos(2 * np.pi * x / 4 + 0.3)
          - 0.25 * np.sin(2 * np.pi * y / 5 + 1.1) * (2 * np.pi / 7) * np.sin(2 * np.pi * x / 7))
    gy = 0.25 * (2 * np.pi / 5) * np.cos(2 * np.pi * y / 5 + 1.1) * np.cos(2 * np.pi * x / 7)
    return np.stack([gx, gy, np.zeros_like(gx)], -1)


def textured_plane(n, seed):
    """points uniform in [-6, 6]^2 on z = 0 (n, 4), normals (0, 0, 1, 0) (n, 4), intensities (n,): float32"""
    xy = np.random.RandomState(seed).uniform(-6.0, 6.0, size=(n, 2))
    pts = np.ones((n, 4), np.float32)
    pts[:, :2], pts[:, 2] = xy.astype(np.float32), 0.0
    nrm = np.zeros((n, 4), np.float32)
    nrm[:, 2] = 1.0
    inten = plane_intensity(pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)).astype(np.float32)
    return pts, nrm, inten


PLANE_T_TRUE = pose(rotation([0, 0, 1], np.deg2rad(2.0)), [0.3, -0.2, 0.05])


def plane_scene():
    """target textured_plane(3000, 1); source textured_plane(1500, 2) moved by the inverse of PLANE_T_TRUE, which is therefore the
    pose that aligns the source to the target. -> dict of float32 arrays"""
    tp, tn, ti = textured_plane(3000, 1)
    sp_, sn, si = textured_plane(1500, 2)
    Tinv = np.linalg.inv(PLANE_T_TRUE)
    src = transform32(Tinv, sp_)
    snr = np.zeros_like(sn)
    snr[:, :3] = (sn[:, :3].astype(np.float64) @ Tinv[:3, :3].T).astype(np.float32)
    return dict(tgt=tp, tgt_normals=tn, tgt_intensities=ti, src=src, src_normals=snr, src_intensities=si)


def pose_errors(T, T_true=PLANE_T_TRUE):
    """(in-plane translation error, full translation error, Frobenius norm of the rotation difference)"""
    T = np.asarray(T, np.float64)
    dt = T[:3, 3] - T_true[:3, 3]
    return float(np.linalg.norm(dt[:2])), float(np.linalg.norm(dt)), float(np.linalg.norm(T[:3, :3] - T_true[:3, :3]))


def curved_sheet(n, seed, T=None):
    """The non-planar family: points on z = 0.3 sin(0.7 x) + 0.2 cos(0.5 y) + 0.02 x y over [-4, 4]^2 with the surface's unit
    normals and intensities in [7.5, 247.5], the whole cloud moved by T (default: a random pose of up to 30 degrees and 5 m drawn
    from the seed). -> points (n, 4), normals (n, 4), intensities (n,), T"""
    rng = np.random.RandomState(seed)
    x, y = rng.uniform(-4.0, 4.0, n), rng.uniform(-4.0, 4.0, n)
    z = 0.3 * np.sin(0.7 * x) + 0.2 * np.cos(0.5 * y) + 0.02 * x * y
    nr = np.stack([-(0.21 * np.cos(0.7 * x) + 0.02 * y), -(-0.1 * np.sin(0.5 * y) + 0.02 * x), np.ones(n)], -1)
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    inten = 127.5 + 90.0 * np.sin(1.3 * x + 0.2) * np.cos(0.9 * y) + 30.0 * np.sin(2.1 * y + x)
    if T is None:
        T = random_pose(rng)
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = (np.stack([x, y, z], -1) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    nrm = np.zeros((n, 4), np.float32)
    nrm[:, :3] = (nr @ T[:3, :3].T).astype(np.float32)
    return pts, nrm, inten.astype(np.float32), T


def sheet_pair(n_src, n_tgt, seed):
    """A source and a target sample of the curved sheet for the linearisation tests: the source lies in the sheet's own frame, the
    target in a random one (up to 30 degrees and 5 m), and T takes the source onto the target up to 2 cm and 0.5 degrees, so
    that residuals are small but not zero. -> dict with the k = 1 correspondences of T * source in the target"""
    rng = np.random.RandomState(seed)
    tgt, tnrm, tint, Tt = curved_sheet(n_tgt, seed + 1)
    Ts = np.eye(4)
    src, _, sint, _ = curved_sheet(n_src, seed + 2, T=Ts)
    off = se3_exp(np.r_[rng.uniform(-1, 1, 3) * np.deg2rad(0.5), rng.uniform(-0.02, 0.02, 3)])
    T = (Tt @ off @ np.linalg.inv(Ts)).astype(np.float32)  # the pose the library gets: float32
    sint = (sint + rng.uniform(-3.0, 3.0, n_src)).astype(np.float32)  # the two scans do not see the same intensity exactly
    q = transform32(T.astype(np.float64), src)
    idx, d2 = nearest(q, tgt)
    return dict(src=src, src_intensities=sint, tgt=tgt, tgt_normals=tnrm, tgt_intensities=tint, T=T, nn_idx=idx, nn_d2=d2)


# ------------------------------------------------------------------------------------------------------------ step 1: gradients
def gradient_model(points, normals, intensities, knn):
    """sp_intensity_gradient in float64 on float32 inputs. -> dict: rows (n, 4) with NaN in column 3 for invalid rows, valid (n,),
    M (n, 3, 3), g (n, 3), m (n,), det (n,)"""
    P = np.asarray(points, np.float64)[:, :3]
    N = np.asarray(normals, np.float64)[:, :3]
    I = np.asarray(intensities, np.float64)
    idx = np.asarray(knn, np.int64)
    n = len(P)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (idx >= 0) & (idx < n) & (idx != np.arange(n)[:, None])
        j = np.where(ok, idx, 0)
        Pj, Ij = P[j], I[j]
        ok &= np.isfinite(Ij) & np.isfinite(Pj).all(-1)
        e = np.where(ok[..., None], Pj - P[:, None, :], 0.0)
        dI = np.where(ok, Ij - I[:, None], 0.0)
        u = e - (e * N[:, None, :]).sum(-1, keepdims=True) * N[:, None, :]
        u = np.where(ok[..., None], u, 0.0)
        m = ok.sum(1)
        M = np.einsum("nki,nkj->nij", u, u) + (m.astype(np.float64) ** 2)[:, None, None] * N[:, :, None] * N[:, None, :]
        g = np.einsum("nki,nk->ni", u, dI)
        det = np.linalg.det(np.where(np.isfinite(M), M, 0.0))
        det = np.where(np.isfinite(M).all((1, 2)), det, np.nan)
        valid = (m >= 3) & np.isfinite(I) & np.isfinite(N).all(1) & (np.abs(det) >= DET_MIN)
    rows = np.zeros((n, 4))
    rows[:, 3] = np.nan
    if valid.any():
        d = np.linalg.solve(M[valid], g[valid][..., None])[..., 0]
        d = d - (d * N[valid]).sum(1, keepdims=True) * N[valid]
        fin = np.isfinite(d).all(1)
        rows[valid, :3] = np.where(fin[:, None], d, 0.0)
        rows[valid, 3] = I[valid]
    return dict(rows=rows, valid=valid, M=M, g=g, m=m, det=det)


def gradient_bound_unit(model):
    """eps32 * kappa(M) * (|d64| + |g| / ||M||) per valid row (2-norms): the unit the twin's deviation is measured in"""
    v = model["valid"]
    out = np.full(len(v), np.nan)
    if v.any():
        M, g, d = model["M"][v], model["g"][v], model["rows"][v, :3]
        sv = np.linalg.svd(M, compute_uv=False)
        out[v] = EPS32 * (sv[:, 0] / sv[:, -1]) * (np.linalg.norm(d, axis=1) + np.linalg.norm(g, axis=1) / sv[:, 0])
    return out


# ------------------------------------------------------------------------------------------------------------ step 2: the term
def robust_weight(loss, r, s):
    r = np.asarray(r, np.float64)
    nr = r / s
    with np.errstate(divide="ignore", invalid="ignore"):
        if loss == "NONE":
            w = np.ones_like(r)
        elif loss == "HUBER":
            w = np.minimum(1.0, 1.0 / nr)
        elif loss == "TUKEY":
            w = np.where(nr >= 1.0, 0.0, (1.0 - nr * nr) ** 2)
        elif loss == "CAUCHY":
            w = 1.0 / (1.0 + nr * nr)
        else:
            w = 1.0 / (1.0 + nr * nr) ** 2
    return np.where(r <= 1e-8, 1.0, w)


def robust_error(loss, r, s):
    with np.errstate(invalid="ignore", over="ignore"):
        return _robust_error(loss, np.asarray(r, np.float64), s)


def _robust_error(loss, r, s):
    if loss == "HUBER":
        return np.where(r <= s, 0.5 * r * r, s * (r - 0.5 * s))
    if loss == "TUKEY":
        return np.where(r <= s, (s * s / 6.0) * (1.0 - (1.0 - np.minimum(r * r / (s * s), 1.0)) ** 3), s * s / 6.0)
    if loss == "CAUCHY":
        return 0.5 * s * s * np.log1p(r * r / (s * s))
    if loss == "GEMAN_MCCLURE":
        return 0.5 * (s * s * r * r) / (s * s + r * r)
    return 0.5 * r * r


def term_mask(src_intensities, tgt_rows, nn_idx, nn_d2, max_distance):
    """which points add to the sums (the library's rejection list; max^2 formed in float32 as the library forms it)"""
    idx = np.asarray(nn_idx, np.int64)
    max_d2 = np.float32(max_distance) * np.float32(max_distance)
    with np.errstate(invalid="ignore"):
        ok = (idx >= 0) & ~(np.asarray(nn_d2, np.float32) > max_d2)
    ok &= ~np.isnan(np.asarray(tgt_rows, np.float32)[np.where(idx >= 0, idx, 0), 3])
    return ok & np.isfinite(np.asarray(src_intensities, np.float32))


def term_model(src, src_intensities, tgt, tgt_rows, nn_idx, nn_d2, T, loss="NONE", scale=1.0, max_distance=np.inf):
    """sp_photometric_linearize in float64 on float32 inputs (T: 4x4, row-major numpy). -> dict: rows (n, 28), r (n,), J (n, 6),
    w (n,), mask (n,), A (n,) the magnitude the residual's rounding is relative to, and the float64 sums"""
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    mask = term_mask(src_intensities, tgt_rows, nn_idx, nn_d2, max_distance)
    idx = np.where(np.asarray(nn_idx) >= 0, nn_idx, 0).astype(np.int64)
    s = np.asarray(src, np.float64)[:, :3]
    Is = np.asarray(src_intensities, np.float64)
    tp = np.asarray(tgt, np.float64)[idx, :3]
    row = np.asarray(tgt_rows, np.float64)[idx]
    d, It = row[:, :3], row[:, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        q = s @ R.T + t
        r = (It + (d * (q - tp)).sum(1)) - Is
        v = d @ R  # R^T d
        J = np.concatenate([np.cross(s, v), v], 1)  # d^T [-R S | R] = [s x v | v]
        a = np.abs(r)
        w, e = robust_weight(loss, a, scale), robust_error(loss, a, scale)
        iu = np.triu_indices(6)
        rows = np.concatenate([w[:, None] * J[:, iu[0]] * J[:, iu[1]], w[:, None] * J * r[:, None], e[:, None]], 1)
        A = np.linalg.norm(d, axis=1) * (np.linalg.norm(s @ R.T, axis=1) + np.linalg.norm(t) + np.linalg.norm(tp, axis=1)) \
            + np.abs(It) + np.abs(Is)
    rows = np.where(mask[:, None], rows, 0.0)
    return dict(rows=rows, r=r, J=J, w=w, mask=mask, A=A, sums=rows.sum(0), inlier=int(mask.sum()))


def unpack_linearized(lin):
    """a library sp_linearized (ctypes) -> (28 float32 in the kLinTerms order, inlier)"""
    H = np.array(lin.H, np.float32).reshape(6, 6)
    iu = np.triu_indices(6)
    return np.concatenate([H[iu], np.array(lin.b, np.float32), [np.float32(lin.error)]]).astype(np.float32), int(lin.inlier)


# ------------------------------------------------------------------------------------------------------------ the aligner
def align_f64(src, src_intensities, tgt, tgt_normals, tgt_intensities, weight, k=10, max_distance=1.5, iterations=30,
              damping=1.0, T0=None, brute_force=False, crit=1e-9):
    """Point-to-plane + photometric Gauss-Newton in float64 (H + damping I, the library's gn_lambda), target gradients from
    gradient_model over the k nearest neighbours, nearest-neighbour correspondences re-found every iteration.
    -> (T, iterations used)"""
    from scipy.spatial import cKDTree

    S = np.asarray(src, np.float64)[:, :3]
    Is = np.asarray(src_intensities, np.float64)
    Pt = np.asarray(tgt, np.float64)[:, :3]
    Nt = np.asarray(tgt_normals, np.float64)[:, :3]
    if brute_force:
        d2 = ((Pt[:, None, :] - Pt[None, :, :]) ** 2).sum(-1)
        knn = np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.int32)
    else:
        knn = knn_self(tgt, k)
    rows = gradient_model(tgt, tgt_normals, tgt_intensities, knn)["rows"]
    tree = None if brute_force else cKDTree(Pt)
    T = np.eye(4) if T0 is None else np.asarray(T0, np.float64).copy()
    used = 0
    for it in range(iterations):
        R, t = T[:3, :3], T[:3, 3]
        q = S @ R.T + t
        if brute_force:
            dd = ((q[:, None, :] - Pt[None, :, :]) ** 2).sum(-1)
            idx = dd.argmin(1)
            dist = np.sqrt(dd[np.arange(len(q)), idx])
        else:
            dist, idx = tree.query(q, k=1)
        ok = dist <= max_distance
        Jq = np.concatenate([-R @ skew(S), np.broadcast_to(R, (len(S), 3, 3))], 2)  # dq / dxi = [-R S | R], (n, 3, 6)
        n_t = Nt[idx]
        rg = (n_t * (q - Pt[idx])).sum(1)
        Jg = np.einsum("ni,nij->nj", n_t, Jq)
        H = np.einsum("n,ni,nj->ij", ok.astype(np.float64), Jg, Jg)
        b = np.einsum("n,ni,n->i", ok.astype(np.float64), Jg, rg)
        if weight > 0:
            d, It = rows[idx, :3], rows[idx, 3]
            okp = ok & ~np.isnan(It) & np.isfinite(Is)
            ri = np.where(okp, (It + (d * (q - Pt[idx])).sum(1)) - Is, 0.0)
            Ji = np.einsum("ni,nij->nj", np.where(okp[:, None], d, 0.0), Jq)
            H += weight * np.einsum("ni,nj->ij", Ji, Ji)
            b += weight * np.einsum("ni,n->i", Ji, ri)
        delta = np.linalg.solve(H + damping * np.eye(6), -b)
        T = T @ se3_exp(delta)
        used = it + 1
        if np.linalg.norm(delta[:3]) < crit and np.linalg.norm(delta[3:]) < crit:
            break
    return T, used
