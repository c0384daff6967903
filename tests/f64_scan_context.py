"""Numpy model of Scan Context place recognition (csrc/place_recognition.hip; the definitions are include/sycl_points_amd.h's).

The descriptor is modelled in float32, operation for operation (numpy's float32 arithmetic rounds each product, sum and square
root once, as the library's uncontracted f32 does), so the host twin and the device must reproduce it bit for bit. Normalisation,
shifted distances and guesses are modelled in float64: the search is held against them within a stated tolerance.
The cases the CPU and the GPU test share are here too (descriptor_cases)."""
import numpy as np

F32 = np.float32
DEFAULTS = dict(rings=20, sectors=60, max_range=80.0, sensor_height=2.0)
SHAPES = ((1, 4), (7, 30), (20, 60), (32, 64))  # rings x sectors


def params(rings=20, sectors=60, max_range=80.0, sensor_height=2.0):
    return dict(rings=int(rings), sectors=int(sectors), max_range=float(F32(max_range)), sensor_height=float(F32(sensor_height)))


# ------------------------------------------------------------------------------------------------------------ descriptor
def boundaries(sectors):
    """c_k, s_k = float32(cos(phi_k)), float32(sin(phi_k)), phi_k = -pi + 2 pi k / sectors in double"""
    k = np.arange(sectors, dtype=np.float64)
    phi = -np.pi + 2.0 * np.pi * k / float(sectors)
    return np.cos(phi).astype(F32), np.sin(phi).astype(F32)


def bins(points, p):
    """Per point: kept (not skipped), ring, sector, value — float32 arithmetic in the header's order."""
    P = np.ascontiguousarray(points, F32).reshape(-1, 4)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    rings, sectors, h = p["rings"], p["sectors"], p["sectors"] // 2
    c, s = boundaries(sectors)
    with np.errstate(all="ignore"):
        r2 = x * x + y * y
        r = np.sqrt(r2)
        kept = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (r2 != 0) & (r < F32(p["max_range"]))
        scale = F32(float(rings) / float(F32(p["max_range"])))
        scaled = np.where(kept, r * scale, F32(0))
        ring = np.minimum(rings - 1, np.floor(scaled).astype(np.int64))
        ge = c[None, :] * y[:, None] >= s[None, :] * x[:, None]
        upper = y >= 0  # (-0.0 too)
        sector = np.where(upper, h + ge[:, h + 1:].sum(1), ge[:, 1:h].sum(1))
        t = z + F32(p["sensor_height"])
        value = np.where(t > 0, t, F32(0)).astype(F32)
    return kept, ring, sector, value


def descriptor(points, p):
    """rings x sectors float32: the maximum value per bin, 0 for an empty bin"""
    kept, ring, sector, value = bins(points, p)
    D = np.zeros((p["rings"], p["sectors"]), F32)
    np.maximum.at(D, (ring[kept], sector[kept]), value[kept])
    return D


# ---------------------------------------------------------------------------------------------------------------- search
def normalise(D):
    """-> unit columns in float64 (zero columns stay zero), the mask of non-empty columns"""
    D = np.asarray(D, np.float64)
    n = np.sqrt((D * D).sum(0))
    mask = n != 0
    return np.where(mask, D / np.where(mask, n, 1.0), 0.0), mask


def shift_distances(Q, C):
    """d_s for s = 0 .. sectors - 1 (float64): the query's column (j + s) mod sectors against the candidate's column j"""
    Qh, qm = normalise(Q)
    Ch, cm = normalise(C)
    S = Qh.shape[1]
    G = Qh.T @ Ch  # G[a][b] = Q^[:, a] . C^[:, b]
    j = np.arange(S)
    d = np.ones(S)
    for s in range(S):
        a = (j + s) % S
        n = int((qm[a] & cm).sum())
        if n:
            d[s] = max(0.0, 1.0 - G[a, j].sum() / n)
    return d


def distance(Q, C):
    """-> (min_s d_s, the lowest s attaining it)"""
    d = shift_distances(Q, C)
    s = int(d.argmin())
    return float(d[s]), s


def guesses(sectors, shift, steps):
    """steps poses Rz(-(shift + delta) 2 pi / sectors), delta evenly over [-1/2, 1/2] (0 for one step) -> (steps, 4, 4) float64"""
    out = np.zeros((steps, 4, 4))
    for i in range(steps):
        delta = -0.5 + i / (steps - 1) if steps > 1 else 0.0
        angle = -(float(shift) + delta) * (2.0 * np.pi) / float(sectors)
        c, s = np.cos(angle), np.sin(angle)
        out[i] = np.eye(4)
        out[i][:2, :2] = [[c, -s], [s, c]]
    return out


# ----------------------------------------------------------------------------------------------------------------- cases
def scan(n, seed, spread=60.0):
    """A random cloud that fills the polar grid unevenly: (n, 4) float32, w = 1"""
    rs = np.random.RandomState(seed)
    P = np.ones((n, 4), F32)
    P[:, :2] = rs.normal(0.0, spread / 2.5, (n, 2))
    P[:, 2] = rs.uniform(-3.0, 12.0, n)
    return P


def boundary_points(p):
    """Points exactly on every ring boundary, on both axes, with y = +0.0 and -0.0 for x of either sign, and on every sector
    boundary direction as the table gives it."""
    rings, sectors, R = p["rings"], p["sectors"], float(F32(p["max_range"]))
    rows = []
    for i in range(rings + 1):
        r = R * i / rings
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1), (0.6, 0.8), (-0.6, -0.8)):
            rows.append((r * dx, r * dy, 1.0 + 0.25 * i))
        rows.append((np.nextafter(F32(r), F32(0)), 0.0, 3.0))
        rows.append((np.nextafter(F32(r), F32(np.inf)), -0.0, 4.0))
    for xs in (5.0, -5.0, 0.5 * R, -0.5 * R):
        rows.append((xs, 0.0, 0.5))
        rows.append((xs, -0.0, 0.75))
        rows.append((0.0, xs, 1.5))
        rows.append((-0.0, xs, 1.75))
    c, s = boundaries(sectors)
    for k in range(sectors):
        for rad in (1.0, 0.37 * R):
            rows.append((rad * float(c[k]), rad * float(s[k]), 2.0 + 0.01 * k))
    P = np.ones((len(rows), 4), F32)
    P[:, :3] = np.array(rows, np.float64).astype(F32)
    neg = np.array([np.signbit(row[1]) for row in rows])  # (the cast keeps -0.0; make sure of it)
    P[neg & (P[:, 1] == 0), 1] = F32(-0.0)
    return P


def descriptor_cases():
    """-> list of (name, params, points): the cases of the host check, which the device repeats"""
    out = []
    d = params()
    for n in (1, 63, 64, 65, 4097):
        out.append((f"random_n{n}", d, scan(n, n)))
    for rings, sectors in SHAPES:
        p = params(rings, sectors, 50.0, 1.5)
        out.append((f"shape_{rings}x{sectors}", p, scan(3000, rings * 100 + sectors, spread=45.0)))
        out.append((f"boundaries_{rings}x{sectors}", p, boundary_points(p)))
    skipped = scan(400, 77)
    skipped[0:10, :2] = 0.0                                  # r = 0
    skipped[5, 1] = -0.0
    skipped[10:20, 0], skipped[10:20, 1] = 80.0, 0.0         # r = max_range exactly
    skipped[20:30, 0] = 500.0                                # beyond
    skipped[30, 0], skipped[31, 1], skipped[32, 2] = np.nan, np.nan, np.nan
    skipped[33, 0], skipped[34, 1], skipped[35, 2] = np.inf, -np.inf, np.inf
    skipped[36, 0] = 3e38                                    # x * x overflows
    skipped[37, :3] = (79.99999, 0.0, 9.0)                   # just inside: the last ring
    out.append(("skipped", d, skipped))
    low = scan(500, 78)
    low[:, 2] = np.random.RandomState(3).uniform(-6.0, -1.0, 500)  # z + sensor_height < 0 for most, = 0 for some
    low[:50, 2] = -2.0
    out.append(("negative_values", d, low))
    hot = np.ones((10000, 4), F32)
    rs = np.random.RandomState(9)
    hot[:, 0] = 10.0 + rs.uniform(0, 0.5, 10000)
    hot[:, 1] = 1.0 + rs.uniform(0, 0.05, 10000)
    hot[:, 2] = rs.uniform(0.0, 5.0, 10000)
    out.append(("contention", d, hot))
    return out


def read_ply_xyz(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int([ln for ln in head.split(b"\n") if ln.startswith(b"element vertex")][0].split()[-1])
    a = np.frombuffer(body, dtype="<f4", count=n * 4).reshape(n, 4)
    pts = np.ones((n, 4), F32)
    pts[:, :3] = a[:, :3]
    return pts


def rot_z(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    T = np.eye(4)
    T[:2, :2] = [[c, -s], [s, c]]
    return T


def bundled_clouds(gold, turn_deg=150.0):
    """The raw bundled scans for the end-to-end condition: the query (the source turned by turn_deg about z) and the database's
    four entries in order: random, the target scaled 1.5 x in x and y, the target, the target mirrored (y -> -y)."""
    src, tgt = read_ply_xyz(gold + "/source.ply"), read_ply_xyz(gold + "/target.ply")
    query = src.copy()
    query[:, :3] = (src[:, :3].astype(np.float64) @ rot_z(turn_deg)[:3, :3].T).astype(F32)
    rs = np.random.RandomState(2024)
    rnd = np.ones((50000, 4), F32)
    rnd[:, :2] = rs.uniform(-80.0, 80.0, (50000, 2))
    rnd[:, 2] = rs.uniform(-2.0, 10.0, 50000)
    scaled = tgt.copy()
    scaled[:, :2] *= F32(1.5)
    mirrored = tgt.copy()
    mirrored[:, 1] = -mirrored[:, 1]
    return query, [rnd, scaled, tgt, mirrored]
