"""A numpy model of the compatibility-graph guesses (include/sycl_points_amd.h): float32 for the predicate and
the scores, exactly as the header fixes them (fmaf emulated exactly), integers for C, S and s, float64 Kabsch by SVD for the
poses. It shares no code with the library: tests/test_compat_cpu.py holds the host twins to it bit for bit, and
tests/test_gpu_compat.py the device to the host twins."""
import numpy as np

F = np.float32


def fmaf(a, b, c):
    """fmaf(a, b, c) of float32 arrays with ONE rounding: the product of two float32 is exact in float64; the sum is rounded to
    odd in float64 (TwoSum gives the exact error, an inexact even result moves to its odd neighbour on the error's side), and a
    float64 rounded to odd rounds to the correct float32 (53 >= 24 + 2 bits)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F).astype(np.float64), np.asarray(b, F).astype(np.float64),
                                  np.asarray(c, F).astype(np.float64))
    p = a * b
    s = p + c
    bb = s - p
    with np.errstate(invalid="ignore"):
        err = (p - (s - bb)) + (c - bb)
    s = np.array(s, np.float64)
    fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
    s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))
    return s.astype(F)


def sq_lengths(p):
    """u[a][b] = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) of d = p_a - p_b, float32"""
    p = np.asarray(p, F)[:, :3]
    d = p[:, None, :] - p[None, :, :]
    return fmaf(d[..., 2], d[..., 2], fmaf(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))


def compatibility(cs, ct, tau, min_edge):
    """C (M, M) uint8, step 1 of the header"""
    t2, e2 = F(tau) * F(tau), F(min_edge) * F(min_edge)
    u, v = sq_lengths(cs), sq_lengths(ct)
    with np.errstate(invalid="ignore", over="ignore"):
        q = (u + v) - t2
        ok = (u > e2) & (v > e2) & ((q < 0) | (q * q < (F(4.0) * u) * v))
    np.fill_diagonal(ok, False)
    return ok.astype(np.uint8)


def second_order(C):
    """S = C o (C C^T) and its row sums, int64 (the float64 product of 0/1 matrices is exact)"""
    Cf = C.astype(np.float64)
    S = (C * (Cf @ Cf.T)).astype(np.int64)
    return S, S.sum(1)


def top(values, n):
    """the indices of the n largest positive values, value descending, index ascending"""
    order = np.lexsort((np.arange(len(values)), -values.astype(np.int64)))
    return [int(i) for i in order[:n] if values[i] > 0]


def seeds_and_lists(cs, ct, tau, min_edge, seeds, k):
    """steps 1-4: (degree, s, seed indices, one companion list per seed)"""
    C = compatibility(cs, ct, tau, min_edge)
    S, s = second_order(C)
    seed_idx = top(s, seeds)
    return C.sum(1).astype(np.int64), s, seed_idx, [top(S[a], k) for a in seed_idx]


def spans_a_plane(p):
    ev = np.linalg.eigvalsh((p - p.mean(0)).T @ (p - p.mean(0)))
    return bool(np.isfinite(ev).all() and ev[2] > 0 and ev[1] > 1e-10 * ev[2])


def kabsch(ps, pt):
    """the least-squares rigid pose taking ps onto pt (float64, SVD), None for a degenerate set"""
    ps, pt = np.asarray(ps, np.float64), np.asarray(pt, np.float64)
    if not (np.isfinite(ps).all() and np.isfinite(pt).all() and spans_a_plane(ps) and spans_a_plane(pt)):
        return None
    ms, mt = ps.mean(0), pt.mean(0)
    U, _, Vt = np.linalg.svd((ps - ms).T @ (pt - mt))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, mt - R @ ms
    return T


def poses(cs, ct, seed_idx, lists):
    """step 5: (poses, the seed rank of each)"""
    out, ranks = [], []
    for r, (a, companions) in enumerate(zip(seed_idx, lists)):
        if len(companions) < 2:
            continue
        ids = [a] + list(companions)
        T = kabsch(np.asarray(cs, np.float64)[ids, :3], np.asarray(ct, np.float64)[ids, :3])
        if T is not None:
            out.append(T), ranks.append(r)
    return np.array(out).reshape(-1, 4, 4), np.array(ranks, np.int64)


def scores(cs, ct, T, inlier_distance):
    """step 6 in the float32 expression of sp_pose_score / sp_ransac_score; T (P, 4, 4) is rounded to float32 first"""
    T = np.asarray(T, np.float64).reshape(-1, 4, 4).astype(F)
    cs, ct = np.asarray(cs, F), np.asarray(ct, F)
    x, y, z = cs[None, :, 0], cs[None, :, 1], cs[None, :, 2]
    r = [fmaf(T[:, a, 2, None], z, fmaf(T[:, a, 1, None], y, fmaf(T[:, a, 0, None], x, T[:, a, 3, None]))) - ct[None, :, a] for a in range(3)]
    d2 = fmaf(r[2], r[2], fmaf(r[1], r[1], r[0] * r[0]))
    with np.errstate(invalid="ignore"):
        return (d2 < F(inlier_distance) * F(inlier_distance)).sum(1).astype(np.int64)


def guesses(cs, ct, tau=0.1, min_edge=0.0, seeds=64, k=16, inlier_distance=1.0, count=64):
    """steps 1-7: (poses best first, their seed ranks, their scores)"""
    _, _, seed_idx, lists = seeds_and_lists(cs, ct, tau, min_edge, seeds, k)
    T, ranks = poses(cs, ct, seed_idx, lists)
    if len(T) == 0:
        return T, ranks, np.zeros(0, np.int64)
    sc = scores(cs, ct, T, inlier_distance)
    order = [int(i) for i in np.argsort(-sc, kind="stable") if sc[i] > 0][:count]
    return T[order], ranks[order], sc[order]


def pose_errors(T, T_true):
    """(translation difference, Frobenius norm of the rotation difference)"""
    T, T_true = np.asarray(T, np.float64), np.asarray(T_true, np.float64)
    return float(np.linalg.norm(T[:3, 3] - T_true[:3, 3])), float(np.linalg.norm(T[:3, :3] - T_true[:3, :3]))


# ------------------------------------------------------------------------------------------------------- synthetic matches
def hall_points(rs, n, size=(60.0, 40.0, 6.0)):
    """n points on the floor and the four walls of a hall, by area"""
    lx, ly, lz = size
    areas = np.array([lx * ly, lx * lz, lx * lz, ly * lz, ly * lz])
    face = rs.choice(5, n, p=areas / areas.sum())
    a, b = rs.uniform(size=n), rs.uniform(size=n)
    p = np.zeros((n, 3))
    p[face == 0] = np.c_[a * lx, b * ly, 0 * a][face == 0]
    p[face == 1] = np.c_[a * lx, 0 * a, b * lz][face == 1]
    p[face == 2] = np.c_[a * lx, 0 * a + ly, b * lz][face == 2]
    p[face == 3] = np.c_[0 * a, a * ly, b * lz][face == 3]
    p[face == 4] = np.c_[0 * a + lx, a * ly, b * lz][face == 4]
    return p


def random_pose(rs):
    """any yaw, about 0.1 rad of tilt, 5 m of translation"""
    yaw = rs.uniform(-np.pi, np.pi)
    tilt = rs.normal(0.0, 0.1, 2)
    cz, sz = np.cos(yaw), np.sin(yaw)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    cx, sx = np.cos(tilt[0]), np.sin(tilt[0])
    cy, sy = np.cos(tilt[1]), np.sin(tilt[1])
    Rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    d = rs.normal(size=3)
    T[:3, 3] = 5.0 * d / np.linalg.norm(d)
    return T


def hall_matches(m, inliers, seed, noise=0.03):
    """m matches in a hall: the first `inliers` (after a fixed shuffle) are moved by a random pose with 3 cm of noise, the others
    pair a random scene point with another random scene point moved by the same pose -> (cs, ct (m, 4) float32, T_true, mask)"""
    rs = np.random.RandomState(seed)
    T = random_pose(rs)
    src = hall_points(rs, m)
    tgt_scene = hall_points(rs, m)
    mask = np.zeros(m, bool)
    mask[rs.permutation(m)[:inliers]] = True
    tgt = np.where(mask[:, None], src + rs.normal(0.0, noise, (m, 3)), tgt_scene) @ T[:3, :3].T + T[:3, 3]
    cs, ct = np.ones((m, 4), F), np.ones((m, 4), F)
    cs[:, :3], ct[:, :3] = src, tgt
    return cs, ct, T, mask
