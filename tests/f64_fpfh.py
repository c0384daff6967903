"""Float64 numpy model of the global registration chain (include/sycl_points_amd.h, "global registration"): SPFH
counts, FPFH rows, nearest neighbours in descriptor space, mutual matches, the counter-based triplet generator, the hypothesis
gates, poses and scores, and the selection of the best hypotheses. Written from the formulas of the header, vectorised; it shares
no code with the library. Test infrastructure: imported by tests/test_global_registration_cpu.py and
tests/test_gpu_global_registration.py."""
import numpy as np

BINS, STRIDE = 33, 36
U64 = np.uint64


# ------------------------------------------------------------------------------------------------------------ preparation
def read_ply_xyz(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int([ln for ln in head.split(b"\n") if ln.startswith(b"element vertex")][0].split()[-1])
    a = np.frombuffer(body, dtype="<f4", count=n * 4).reshape(n, 4)
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = a[:, :3]
    return pts


def rot_z(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    T = np.eye(4)
    T[:2, :2] = [[c, -s], [s, c]]
    return T


def voxel_centroids(xyz, size):
    """One point per occupied voxel of edge `size`: the mean of its points (float64), in key order."""
    xyz = np.asarray(xyz, np.float64)
    keys = np.floor(xyz / size).astype(np.int64)
    _, inv, cnt = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    out = np.zeros((len(cnt), 3))
    np.add.at(out, inv, xyz)
    return out / cnt[:, None]


def knn_self(xyz, k):
    """k nearest neighbours of every point among all points (itself included), ascending: indices int32, squared distances."""
    xyz = np.asarray(xyz, np.float64)
    d2 = ((xyz[:, None, :] - xyz[None, :, :]) ** 2).sum(-1)
    k = min(k, len(xyz))
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int32), np.take_along_axis(d2, idx, 1)


def pca_normals(xyz, idx):
    """Unit normals from the neighbourhoods `idx`, turned towards the origin (the sensor)."""
    xyz = np.asarray(xyz, np.float64)
    nb = xyz[idx]
    c = nb - nb.mean(1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", c, c)
    _, v = np.linalg.eigh(cov)
    nrm = v[:, :, 0]
    flip = (nrm * xyz).sum(1) > 0
    nrm[flip] *= -1
    return nrm


# ------------------------------------------------------------------------------------------------------------------ FPFH
def spfh_pairs(points, normals, idx):
    """Per list entry (n, k): `nb` it is a neighbour (j >= 0, j != i), `ok` the pair is binned, b1 b2 b3 its bins, `uncertain` a
    scaled feature lies within 1e-4 of an integer or |v| < 1e-3 dist (float64 cannot vouch for the float32 bin)."""
    P = np.asarray(points, np.float64)[:, :3]
    N = np.asarray(normals, np.float64)[:, :3]
    idx = np.asarray(idx)
    n, k = idx.shape
    i = np.arange(n)[:, None]
    nb = (idx >= 0) & (idx < n) & (idx != i)
    j = np.where(nb, idx, 0)
    with np.errstate(all="ignore"):
        d = P[j] - P[i]
        dist = np.linalg.norm(d, axis=2)
        ni = np.broadcast_to(N[i], d.shape)
        nj = N[j]
        f3 = (ni * d).sum(2) / dist
        v = np.cross(d, ni)
        vn = np.linalg.norm(v, axis=2)
        v = v / vn[:, :, None]
        w = np.cross(ni, v)
        f2 = (v * nj).sum(2)
        f1 = np.arctan2((w * nj).sum(2), (ni * nj).sum(2))
        s1, s2, s3 = 11 * (f1 + np.pi) / (2 * np.pi), 11 * (f2 + 1) / 2, 11 * (f3 + 1) / 2
        ok = nb & (dist > 0) & (vn > 0) & np.isfinite(s1) & np.isfinite(s2) & np.isfinite(s3) & np.isfinite(dist) & np.isfinite(vn)
        s = np.stack([s1, s2, s3])
        s = np.where(ok[None], s, 0.0)
        bins = np.clip(np.floor(s), 0, 10).astype(np.int64)
        near = (np.abs(s - np.round(s)) < 1e-4).any(0)
        uncertain = ok & (near | (vn < 1e-3 * dist))
        # a pair float64 skips or bins on the very edge of |v| == 0 / dist == 0 is the float32 side's to decide as well
        uncertain |= nb & ~ok & np.isfinite(dist) & (dist > 0) & np.isfinite(vn) & (vn < 1e-3 * dist)
    return dict(nb=nb, ok=ok, b1=bins[0], b2=bins[1], b3=bins[2], uncertain=uncertain)


def spfh_counts(points, normals, idx):
    """-> counts (n, 33) int64, m (n,), uncertain pairs per row (n,), pairs per row (n,)"""
    pr = spfh_pairs(points, normals, idx)
    n = len(points)
    counts = np.zeros((n, BINS), np.int64)
    rows = np.broadcast_to(np.arange(n)[:, None], pr["ok"].shape)
    for off, b in ((0, pr["b1"]), (11, pr["b2"]), (22, pr["b3"])):
        np.add.at(counts, (rows[pr["ok"]], off + b[pr["ok"]]), 1)
    return counts, pr["nb"].sum(1), pr["uncertain"].sum(1), pr["nb"].sum(1)


def fpfh_from_counts(counts, m, idx, d2):
    """FPFH rows (n, 33) in float64 from SPFH counts: SPFH = count * 100 / m, weighted by 1 / d2 over the neighbours, each group of
    11 bins scaled to sum 100."""
    counts, m = np.asarray(counts, np.float64), np.asarray(m, np.float64)
    idx, d2 = np.asarray(idx), np.asarray(d2, np.float64)
    n = len(counts)
    with np.errstate(all="ignore"):
        spfh = np.where(m[:, None] > 0, counts * (100.0 / m[:, None]), 0.0)
        nb = (idx >= 0) & (idx < n) & (idx != np.arange(n)[:, None]) & (d2 != 0)
        w = np.where(nb, 1.0 / d2, 0.0)
        F = np.einsum("nk,nkb->nb", w, spfh[np.where(nb, idx, 0)])
        g = F.reshape(n, 3, 11)
        s = g.sum(2, keepdims=True)
        g = np.where(s != 0, g * (100.0 / s), 0.0)
    return g.reshape(n, BINS)


def fpfh(points, normals, idx, d2):
    counts, m, _, _ = spfh_counts(points, normals, idx)
    return fpfh_from_counts(counts, m, idx, d2)


# ----------------------------------------------------------------------------------------------------------------- match
def distances(a, b):
    a, b = np.asarray(a, np.float64)[:, :BINS], np.asarray(b, np.float64)[:, :BINS]
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def match(a, b):
    """-> (index of the nearest row of b, lowest index on ties; its squared distance), -1 / inf for an empty b"""
    if len(b) == 0:
        return np.full(len(a), -1, np.int64), np.full(len(a), np.inf)
    D = distances(a, b)
    j = D.argmin(1)
    return j, D[np.arange(len(a)), j]


def mutual(src, tgt):
    """-> (M, 2) pairs (i, j) in ascending i with match(tgt -> src)[match(src -> tgt)[i]] == i"""
    if len(src) == 0 or len(tgt) == 0:
        return np.zeros((0, 2), np.int64)
    D = distances(src, tgt)
    s2t, t2s = D.argmin(1), D.argmin(0)
    i = np.arange(len(src))
    keep = t2s[s2t] == i
    return np.stack([i[keep], s2t[keep]], 1)


# ---------------------------------------------------------------------------------------------------------------- RANSAC
def splitmix64(z):
    z = np.asarray(z, U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def triplets(seed, hypotheses, m, first=0):
    """(hypotheses, 3) indices into the m matches: index_j = ((splitmix64(seed + 3 h + j) >> 32) * m) >> 32"""
    h = np.arange(first, first + hypotheses, dtype=U64)
    with np.errstate(over="ignore"):
        z = U64(seed) + U64(3) * h[:, None] + np.arange(3, dtype=U64)[None, :]
        r = splitmix64(z)
        return (((r >> U64(32)) * U64(m)) >> U64(32)).astype(np.int64)


def _frames(p):
    """p (H, 3, 3) triangles -> frames (H, 3, 3) with columns e1 e2 e3, centroids (H, 3)"""
    e, f = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    with np.errstate(all="ignore"):
        e1 = e / np.linalg.norm(e, axis=1, keepdims=True)
        n = np.cross(e1, f)
        e3 = n / np.linalg.norm(n, axis=1, keepdims=True)
    e2 = np.cross(e3, e1)
    return np.stack([e1, e2, e3], 2), p.mean(1)


def hypotheses(cs, ct, trip, min_edge, edge_ratio):
    """-> valid (H,), R (H, 3, 3), t (H, 3), near (H,): a gate quantity lies within relative 1e-4 of its threshold"""
    cs, ct = np.asarray(cs, np.float64)[:, :3], np.asarray(ct, np.float64)[:, :3]
    ps, pt = cs[trip], ct[trip]
    distinct = (trip[:, 0] != trip[:, 1]) & (trip[:, 0] != trip[:, 2]) & (trip[:, 1] != trip[:, 2])
    valid, near = distinct.copy(), np.zeros(len(trip), bool)

    def gate(value, threshold):  # value >= threshold passes
        nonlocal valid, near
        valid &= value >= threshold
        near |= np.abs(value - threshold) <= 1e-4 * np.maximum(np.abs(threshold), 1e-300)

    with np.errstate(all="ignore"):
        for a, b in ((0, 1), (0, 2), (1, 2)):
            ls, lt = np.linalg.norm(ps[:, b] - ps[:, a], axis=1), np.linalg.norm(pt[:, b] - pt[:, a], axis=1)
            valid &= ls > min_edge
            near |= np.abs(ls - min_edge) <= 1e-4 * max(min_edge, 1e-300)
            gate(np.minimum(ls, lt), edge_ratio * np.maximum(ls, lt))
        for p in (ps, pt):
            e, f = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
            c = np.cross(e, f)
            gate((c * c).sum(1), 0.04 * (e * e).sum(1) * (f * f).sum(1))
        Fs, cen_s = _frames(ps)
        Ft, cen_t = _frames(pt)
        R = np.einsum("hac,hbc->hab", Ft, Fs)
        t = cen_t - np.einsum("hab,hb->ha", R, cen_s)
    valid &= np.isfinite(R).all((1, 2)) & np.isfinite(t).all(1)
    near &= distinct
    return valid, R, t, near


def residuals2(cs, ct, R, t, chunk=2048):
    """squared residuals (H, M) of every match under every pose"""
    cs, ct = np.asarray(cs, np.float64)[:, :3], np.asarray(ct, np.float64)[:, :3]
    out = np.empty((len(R), len(cs)))
    for a in range(0, len(R), chunk):
        x = np.einsum("hab,mb->hma", R[a:a + chunk], cs) + t[a:a + chunk, None, :] - ct[None]
        out[a:a + chunk] = (x * x).sum(2)
    return out


def scores(cs, ct, hyps, seed, tau, min_edge, edge_ratio):
    """-> scores (H,) int64 and the pieces: valid, near, r2 (H, M), R, t"""
    m = len(cs)
    if m < 3:
        z = np.zeros(hyps, np.int64)
        return z, dict(valid=z.astype(bool), near=z.astype(bool), r2=np.zeros((hyps, m)), R=None, t=None)
    trip = triplets(seed, hyps, m)
    valid, R, t, near = hypotheses(cs, ct, trip, min_edge, edge_ratio)
    with np.errstate(all="ignore"):
        r2 = residuals2(cs, ct, np.where(valid[:, None, None], R, 0.0), np.where(valid[:, None], t, 0.0))
    sc = np.where(valid, (r2 < tau * tau).sum(1), 0)
    return sc.astype(np.int64), dict(valid=valid, near=near, r2=r2, R=R, t=t, trip=trip)


def select(score, guesses):
    """the hypotheses with the `guesses` highest nonzero scores, ties to the lower h"""
    score = np.asarray(score, np.int64)
    h = np.nonzero(score)[0]
    order = h[np.lexsort((h, -score[h]))]
    return order[:guesses]


def poses(cs, ct, seed, hyp):
    """4x4 poses of the hypotheses `hyp` (no gates)"""
    hyp = np.asarray(hyp, np.int64)
    out = np.tile(np.eye(4), (len(hyp), 1, 1))
    if len(hyp) == 0:
        return out
    cs, ct = np.asarray(cs, np.float64)[:, :3], np.asarray(ct, np.float64)[:, :3]
    trip = np.concatenate([triplets(seed, 1, len(cs), first=int(h)) for h in hyp])
    Fs, cen_s = _frames(cs[trip])
    Ft, cen_t = _frames(ct[trip])
    R = np.einsum("hac,hbc->hab", Ft, Fs)
    out[:, :3, :3] = R
    out[:, :3, 3] = cen_t - np.einsum("hab,hb->ha", R, cen_s)
    return out


def pose_errors(T, T_true):
    """(translation error, rotation angle) of T against T_true"""
    d = np.linalg.inv(np.asarray(T_true, np.float64)) @ np.asarray(T, np.float64)
    c = np.clip((np.trace(d[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.linalg.norm(d[:3, 3])), float(np.arccos(c))


def bundled_pair(gold, voxel=1.0, k=20, turn_deg=150.0):
    """The bundled scans as the feasibility check prepared them: voxel centroids, the source turned by `turn_deg` about z around
    the sensor, k-NN lists, 10-NN normals towards the sensor. -> dict(src, tgt: (xyz, normals, idx, d2)), T_true 4x4"""
    import os

    T = np.loadtxt(os.path.join(gold, "T_target_source.txt"))
    Rz = rot_z(turn_deg)
    out = {}
    for name in ("source", "target"):
        xyz = read_ply_xyz(os.path.join(gold, name + ".ply"))[:, :3].astype(np.float64)
        r = np.linalg.norm(xyz, axis=1)
        xyz = voxel_centroids(xyz[(r > 0.5) & (r < 50.0)], voxel)
        if name == "source":
            xyz = xyz @ Rz[:3, :3].T
        xyz = xyz.astype(np.float32).astype(np.float64)
        idx, d2 = knn_self(xyz, k)
        nrm = pca_normals(xyz, idx[:, :10])
        out[name] = (xyz, nrm, idx, d2)
    return out, T @ np.linalg.inv(Rz)
