"""Float64 model of the 15-DoF LiDAR-inertial alignment, written from the mathematics only: numpy.linalg.inv / solve / eigh,
Rodrigues' formula and the matrix logarithm, the block formulas of the ICP embedding, J P J^T, and the definition of Powell's
dog-leg step. No pivoted LDL^T, no quaternions. Every function takes `dt` (float64 by default): tests/test_lio_cpu.py runs the
same formulas in float32 to measure what plain float32 arithmetic costs (K_ref).

Error-state order [dp, dphi, dv, db_a, db_g]; a state is (p, R, v, ba, bg); the ICP system is ordered [d_omega, d_t], body frame."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
POS, ROT, VEL, ACC, GYR = 0, 3, 6, 9, 12


class St:
    def __init__(self, p, R, v, ba, bg, dt=np.float64):
        self.p, self.R, self.v, self.ba, self.bg = (np.asarray(a, dt) for a in (p, R, v, ba, bg))

    @staticmethod
    def unpack(s, dt=np.float64):
        s = np.asarray(s, dt)
        return St(s[0:3], s[3:12].reshape(3, 3).T, s[12:15], s[15:18], s[18:21], dt)

    def pack(self):
        return np.concatenate([self.p, self.R.T.reshape(-1), self.v, self.ba, self.bg])

    def pose(self):
        T = np.eye(4, dtype=self.R.dtype)
        T[:3, :3], T[:3, 3] = self.R, self.p
        return T


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.asarray(w).dtype)


def rodrigues(w):
    w = np.asarray(w)
    dt = w.dtype
    th = np.sqrt(w @ w)
    K = skew(w)
    if th < 1e-4:  # series: the next terms are below 1e-17 relative
        a, b = dt.type(1) - th * th / 6, dt.type(0.5) - th * th / 24
    else:
        a, b = np.sin(th) / th, (1 - np.cos(th)) / (th * th)
    return np.eye(3, dtype=dt) + a * K + b * (K @ K)


def log_so3(R):
    """The rotation vector of R: angle from atan2(|vee(R - R^T)| / 2, (tr R - 1) / 2), axis from the antisymmetric part
    (angles well below pi, which is all the alignment meets)."""
    R = np.asarray(R)
    A = (R - R.T) / 2
    v = np.array([A[2, 1], A[0, 2], A[1, 0]], dtype=R.dtype)
    s = np.sqrt(v @ v)
    c = (np.trace(R) - 1) / 2
    th = np.arctan2(s, c)
    if s < 1e-8:
        return v
    return v * (th / s)


def residual(pred, op):
    return np.concatenate([op.p - pred.p, log_so3(pred.R.T @ op.R), op.v - pred.v, op.ba - pred.ba, op.bg - pred.bg])


def imu_hessian_gradient(pred, op, P):
    H = np.linalg.inv(P)
    return H, H @ residual(pred, op)


def add_icp(H, b, H6, b6, R, w):
    """H, b (15) += w * embedding of the 6x6 ICP system at rotation R"""
    H, b = H.copy(), b.copy()
    Hww, Hwt, Htw, Htt = H6[:3, :3], H6[:3, 3:], H6[3:, :3], H6[3:, 3:]
    H[ROT:ROT + 3, ROT:ROT + 3] += w * Hww
    H[POS:POS + 3, POS:POS + 3] += w * (R @ Htt @ R.T)
    H[POS:POS + 3, ROT:ROT + 3] += w * (R @ Htw)
    H[ROT:ROT + 3, POS:POS + 3] += w * (Hwt @ R.T)
    b[ROT:ROT + 3] += w * b6[:3]
    b[POS:POS + 3] += w * (R @ b6[3:])
    return H, b


def block_filter(Hb, min_per_inlier, weak_scale, inlier):
    lam, V = np.linalg.eigh((Hb + Hb.T) / 2)
    min_info = max(0.0, min_per_inlier) * inlier
    weak = min(max(weak_scale, 0.0), 1.0)
    F = np.zeros((3, 3), Hb.dtype)
    for i in range(3):
        l = max(0.0, lam[i])
        s = 1.0
        if l <= 0.0 or not np.isfinite(l):
            s = 0.0
        elif min_info > 0.0:
            s = max(weak, min(max(l / min_info, 0.0), 1.0))
        F += np.sqrt(min(max(s, 0.0), 1.0)).astype(Hb.dtype) * np.outer(V[:, i], V[:, i])
    return F, lam, min_info


def directional(H, b, inlier, enable, trans_min, rot_min, trans_weak, rot_weak):
    """Returns H, b and the eigenvalues / thresholds the filters used (for branch safety)."""
    if not enable or inlier == 0:
        return H.copy(), b.copy(), None
    H, b = H.copy(), b.copy()
    Hp = H[:6, :6].copy()
    Hp = (Hp + Hp.T) / 2
    F = np.zeros((6, 6), H.dtype)
    F[:3, :3], lt, mt = block_filter(Hp[:3, :3], trans_min, trans_weak, inlier)
    F[3:, 3:], lr, mr = block_filter(Hp[3:, 3:], rot_min, rot_weak, inlier)
    H[:6, :6] = F @ Hp @ F
    b[:6] = F @ F @ b[:6]
    return H, b, ((lt, mt), (lr, mr))


def solve(H, b):
    return -np.linalg.solve(H, b), np.linalg.inv(H)


def retract(x, d):
    dt = x.R.dtype
    return St(x.p + d[POS:POS + 3], x.R @ rodrigues(d[ROT:ROT + 3]), x.v + d[VEL:VEL + 3], x.ba + d[ACC:ACC + 3],
              x.bg + d[GYR:GYR + 3], dt)


def jacobian(T_imu_to_lidar, R_world_lidar, inverse=False):
    T = np.asarray(T_imu_to_lidar)
    dt = T.dtype
    R_li, t_li = T[:3, :3], T[:3, 3]
    t_lidar_in_imu = -R_li.T @ t_li
    R_wi = R_world_lidar @ R_li
    J = np.eye(15, dtype=dt)
    if not inverse:
        J[ROT:ROT + 3, ROT:ROT + 3] = R_li
        J[POS:POS + 3, ROT:ROT + 3] = -R_wi @ skew(t_lidar_in_imu)
    else:
        J[ROT:ROT + 3, ROT:ROT + 3] = R_li.T
        J[POS:POS + 3, ROT:ROT + 3] = R_wi @ skew(t_lidar_in_imu) @ R_li.T
    return J


def transform_covariance(P, T, R, lidar_to_imu):
    J = jacobian(T, R, inverse=bool(lidar_to_imu))
    return J @ P @ J.T


def dogleg(H, g, radius):
    """Powell's dog-leg: the Gauss-Newton point when inside the region, the scaled steepest-descent direction when the Cauchy point is
    outside, else the point of the segment Cauchy -> Gauss-Newton on the boundary. Returns p, |p|, the model reduction, the branch
    (0 GN, 1 scaled Cauchy, 2 segment, 3 no GN point), the two norms and the condition number of H."""
    dt = H.dtype
    eps = dt.type(np.finfo(np.float32).eps)
    has_gn = bool(np.all(np.linalg.eigvalsh((H + H.T) / 2) > 0))
    p_gn = -np.linalg.solve(H, g) if has_gn else np.zeros_like(g)
    n_gn = np.sqrt(p_gn @ p_gn)
    gHg = g @ (H @ g)
    p_sd = -g
    if gHg > eps:
        p_sd = -((g @ g) / gHg) * g
    n_sd = np.sqrt(p_sd @ p_sd)
    if has_gn and n_gn <= radius:
        p, norm, branch = p_gn, n_gn, 0
    elif n_sd >= radius:
        p, norm, branch = (radius / n_sd) * p_sd, dt.type(radius), 1
    elif has_gn:
        d = p_gn - p_sd
        a, bq, c = d @ d, 2 * (p_sd @ d), p_sd @ p_sd - radius * radius
        tau = (-bq + np.sqrt(max(bq * bq - 4 * a * c, 0))) / (2 * a)
        tau = min(max(tau, 0), 1)
        p = p_sd + tau * d
        norm, branch = np.sqrt(p @ p), 2
    else:
        p, norm, branch = p_sd, n_sd, 3
    return p, norm, -(g @ p + (p @ (H @ p)) / 2), branch, n_gn, n_sd


def icp_weight(error, inlier, dim):
    dof = dim * inlier - 6.0
    if dof > 0 and np.isfinite(error) and error >= 0:
        return 1.0 / max(1.0, 2.0 * error / dof)
    return 1.0


def imu_cost(pred, x, H_imu):
    r = residual(pred, x)
    return 0.5 * (r @ (H_imu @ r))


def combined_system(lin, op, pred, H_imu, imu_valid, first, dim, dirw, invalid_reg, dt=np.float64):
    """The 15x15 system of one outer iteration: chi-square weight, embedding, directional weighting, IMU prior (b_imu = 0 in the first
    iteration: the prior is linearised at the prediction) or the regularisation of an invalid one. Returns H, b, weight."""
    w = dt(icp_weight(float(lin["error"]), int(lin["inlier"]), dim))
    H, b = add_icp(np.zeros((15, 15), dt), np.zeros(15, dt), np.asarray(lin["H"], dt), np.asarray(lin["b"], dt), op.R, w)
    H, b, _ = directional(H, b, int(lin["inlier"]), *dirw)
    if imu_valid:
        H = H + H_imu
        if not first:
            b = b + H_imu @ residual(pred, op)
    else:
        for i in range(VEL, 15):
            H[i, i] += invalid_reg
    return H, b, w


def freeze(d, update_bias):
    d = d.copy()
    if not update_bias:
        d[ACC:] = 0
    return d
