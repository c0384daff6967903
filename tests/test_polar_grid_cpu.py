"""PolarGrid's key function on the host (sp_polar_keys_host and the atan2f it is made of, csrc/sp_math.h): accuracy against
float64, the reference's invalid-key rules (filter/polar_downsampling.hpp:30-100) and the argument checks. No GPU."""
import ctypes as C

import numpy as np
import pytest

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
MASK = (1 << 21) - 1
ULP_BOUND = 2.0  # sp_math.h: sp_atan2f is held to 2 ulp of the correctly rounded result


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def atan2f(L, y, x):
    y, x = np.ascontiguousarray(y, np.float32), np.ascontiguousarray(x, np.float32)
    out = np.empty(len(y), np.float32)
    L.sp_internal_atan2f_host(vp(y), vp(x), len(y), vp(out))
    return out


def host_keys(L, pts, coord, d, e, a):
    pts = np.ascontiguousarray(pts, np.float32)
    keys = np.empty(len(pts), np.uint64)
    inv = [float(np.float32(1.0) / np.float32(v)) for v in (d, e, a)]
    rc = L.sp_polar_keys_host(vp(pts), len(pts), coord, *inv, vp(keys))
    assert rc == 0, L.sp_last_error()
    return keys


def ulp_error(got, y, x):
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    ulp = np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64)
    return np.abs(got.astype(np.float64) - ref) / ulp


def test_atan2f_within_two_ulp_over_every_octant(L):
    rs = np.random.RandomState(20)
    n = 1_200_000
    sgn = lambda k: rs.choice(np.float32([-1.0, 1.0]), k)  # noqa: E731
    mag = lambda k: (np.float32(10.0) ** rs.uniform(-44.0, 38.5, k)).astype(np.float32)  # noqa: E731  (subnormal .. huge)
    y, x = np.empty(n, np.float32), np.empty(n, np.float32)
    q = n // 4
    y[:q], x[:q] = rs.uniform(-1, 1, q), rs.uniform(-1, 1, q)                 # unit square: every octant
    y[q:2 * q], x[q:2 * q] = sgn(q) * mag(q), sgn(q) * mag(q)                  # magnitudes from subnormal to near FLT_MAX
    base = (sgn(q) * mag(q)).astype(np.float32)
    y[2 * q:3 * q] = base * (np.float32(1.0) + rs.uniform(-1e-3, 1e-3, q).astype(np.float32)) * sgn(q)  # near the diagonals
    x[2 * q:3 * q] = base
    ang = rs.uniform(-np.pi, np.pi, n - 3 * q)                                  # sensor-like: ranges 0.1 .. 200 m
    r = rs.uniform(0.1, 200.0, n - 3 * q)
    y[3 * q:], x[3 * q:] = (r * np.sin(ang)).astype(np.float32), (r * np.cos(ang)).astype(np.float32)
    got = atan2f(L, y, x)
    err = ulp_error(got, y, x)
    assert np.isfinite(got).all()
    assert err.max() <= ULP_BOUND, (err.max(), y[err.argmax()], x[err.argmax()])
    assert (np.abs(got) <= np.float32(np.pi)).all()


def test_atan2f_signed_zeros_and_axes(L):
    pi, pio2 = np.float32(np.pi), np.float32(np.pi / 2)
    z, nz = np.float32(0.0), np.float32(-0.0)
    cases = [  # (y, x, expected) by C99 F.9.1.4
        (z, z, z), (nz, z, nz), (z, nz, pi), (nz, nz, -pi),
        (z, np.float32(-3.0), pi), (nz, np.float32(-3.0), -pi), (z, np.float32(3.0), z), (nz, np.float32(3.0), nz),
        (np.float32(2.0), z, pio2), (np.float32(2.0), nz, pio2), (np.float32(-2.0), z, -pio2), (np.float32(-2.0), nz, -pio2),
        (np.float32(1.0), np.float32(1.0), np.float32(np.pi / 4)), (np.float32(-1.0), np.float32(-1.0), np.float32(-3 * np.pi / 4)),
        (np.float32(1e-45), np.float32(1.0), np.float32(1e-45)), (np.float32(3e38), np.float32(-1e-38), pio2),
    ]
    y = np.array([c[0] for c in cases], np.float32)
    x = np.array([c[1] for c in cases], np.float32)
    want = np.array([c[2] for c in cases], np.float32)
    got = atan2f(L, y, x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), list(zip(y, x, got, want))


def float64_keys(pts, coord, d, e, a):
    """compute_polar_bit with float64 angles (and float32 r, products as in the library); None where the key is invalid"""
    p = pts.astype(np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r = np.sqrt((x * x + y * y) + z * z)
    h2 = (x * x + y * y) if coord == 0 else (x * x + z * z)
    X, Y, Z = (v.astype(np.float64) for v in (x, y, z))
    if coord == 0:
        az, el = np.arctan2(Y, X), np.arctan2(Z, np.sqrt(h2.astype(np.float64)))
    else:
        az, el = np.arctan2(X, Z), np.arctan2(-Y, np.sqrt(h2.astype(np.float64)))
    inv = [np.float32(1.0) / np.float32(v) for v in (d, e, a)]
    q = [(r * inv[0]).astype(np.float64), el * np.float64(inv[1]), az * np.float64(inv[2])]
    f = [np.floor(v) + (1 << 20) for v in q]
    k = f[0].astype(np.uint64) | (f[1].astype(np.uint64) << np.uint64(21)) | (f[2].astype(np.uint64) << np.uint64(42))
    # points within a few ulp of an angle bin edge may fall on either side: report them
    edge = np.zeros(len(p), bool)
    for v, ang, s in ((q[1], el, inv[1]), (q[2], az, inv[2])):
        band = 4.0 * np.spacing(np.abs(ang).astype(np.float32)).astype(np.float64) * float(s) + 4.0 * np.spacing(np.abs(v).astype(np.float32))
        edge |= np.abs(v - np.round(v)) <= band
    return k, edge


@pytest.mark.parametrize("coord", [0, 1])
def test_host_keys_against_float64_angles(L, coord):
    rs = np.random.RandomState(7 + coord)
    n = 400_000
    ang = rs.uniform(-np.pi, np.pi, n)
    elv = rs.uniform(-0.5, 0.5, n)
    r = rs.uniform(1.0, 80.0, n)
    pts = np.ones((n, 4), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = r * np.cos(elv) * np.cos(ang), r * np.cos(elv) * np.sin(ang), r * np.sin(elv)
    pts[: n // 8, :3] = rs.uniform(-5, 5, (n // 8, 3))
    for d, e, a in ((0.5, np.deg2rad(1.0), np.deg2rad(1.0)), (1.0, np.pi, np.pi), (0.1, 0.01, 0.003)):
        keys = host_keys(L, pts, coord, d, e, a)
        want, edge = float64_keys(pts, coord, d, e, a)
        assert (keys != INVALID).all()
        differ = keys != want
        assert not (differ & ~edge).any(), np.flatnonzero(differ & ~edge)[:10]
        assert differ.sum() <= edge.sum() and edge.mean() < 1e-3, (differ.sum(), edge.sum())
        # the fields decode to the reference layout: DISTANCE bits 0-20, POLAR 21-41, AZIMUTH 42-62
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        r = np.sqrt((x * x + y * y) + z * z)  # float32, the reference's order: the distance field is exact
        dist = (keys & np.uint64(MASK)).astype(np.int64) - (1 << 20)
        assert np.array_equal(dist, np.floor(r * (np.float32(1.0) / np.float32(d))).astype(np.int64))
        assert (keys >> np.uint64(63) == 0).all()


def test_invalid_key_rules(L):
    big = np.float32(3e38)
    pts = np.array([
        [np.nan, 1, 1, 1], [1, np.inf, 1, 1], [1, 1, -np.inf, 1],   # non-finite
        [0, 0, 0, 1], [-0.0, 0, -0.0, 1],                            # r == 0
        [0, 0, 5, 1], [-0.0, 0.0, -2, 1],                            # LIDAR: on the z axis (x^2 + y^2 == 0)
        [1e-30, 1e-30, 1e-30, 1],                                    # every square underflows: r == 0
        [big, 1, 1, 1],                                              # x^2 overflows: r = inf
        [3e6, 0, 1, 1],                                              # distance field past 2^20 at d = 1
        [1, 2, 3, 1],                                                # valid
    ], np.float32)
    k = host_keys(L, pts, 0, 1.0, 0.1, 0.1)
    assert (k[:-1] == INVALID).all() and k[-1] != INVALID
    cam = np.array([[0, 5, 0, 1], [0, -0.0, 0, 1], [0, -3, -0.0, 1], [1, 5, 0, 1], [0, 5, 1, 1]], np.float32)
    kc = host_keys(L, cam, 1, 1.0, 0.1, 0.1)
    assert (kc[:3] == INVALID).all() and (kc[3:] != INVALID).all()   # CAMERA: on the y axis (x^2 + z^2 == 0)
    lid = host_keys(L, cam, 0, 1.0, 0.1, 0.1)
    assert (lid[[0, 2, 3, 4]] != INVALID).all()                       # ... which LIDAR keeps
    # an angle field out of range: azimuth pi / 1e-7 > 2^20 bins
    assert host_keys(L, np.array([[-1, 1e-3, 0, 1]], np.float32), 0, 1.0, 1.0, 1e-7)[0] == INVALID
    assert host_keys(L, np.array([[1, 1e-3, 0, 1]], np.float32), 0, 1.0, 1.0, 1e-7)[0] != INVALID
    # the field range ends exactly at 2^20: d such that r * d_inv == 2^20 - 1 is kept, 2^20 is not
    assert host_keys(L, np.array([[1048575.0, 0, 1, 1]], np.float32), 0, 1.0, 1.0, 1.0)[0] != INVALID
    assert host_keys(L, np.array([[1048576.0, 0, 1, 1]], np.float32), 0, 1.0, 1.0, 1.0)[0] == INVALID


def test_argument_errors(L):
    pts = np.ones((4, 4), np.float32)
    keys = np.zeros(4, np.uint64)
    assert L.sp_polar_keys_host(vp(pts), 4, 2, 1.0, 1.0, 1.0, vp(keys)) == 1
    assert b"coordinate system" in L.sp_last_error()
    assert L.sp_polar_keys_host(vp(pts), 4, -1, 1.0, 1.0, 1.0, vp(keys)) == 1
    for bad in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("inf")), (1.0, float("nan"), 1.0)):
        assert L.sp_polar_keys_host(vp(pts), 4, 0, *bad, vp(keys)) == 1
        assert b"positive" in L.sp_last_error()
    assert L.sp_polar_keys_host(vp(pts), 0, 0, 1.0, 1.0, 1.0, None) == 0
    # the device entry points check the same before touching the device
    assert L.sp_polar_keys(None, 4, 5, 1.0, 1.0, 1.0, None, None) == 1
    assert L.sp_polar_key_box(None, 4, 0, 0.0, 1.0, 1.0, vp(np.zeros(6, np.int32)), None) == 1
    assert L.sp_polar_downsample_report(None, 4, 1, 1.0, -1.0, 1.0, 1, None, None, None, None, None, None, None, None, None, None,
                                        vp(np.zeros(8, np.int32)), None, 0, None) == 1


def test_python_facade_arguments():
    import sycl_points_amd.api as sp

    with pytest.raises(sp.SpError):
        sp.PolarGrid(0.0, 1.0, 1.0)
    with pytest.raises(sp.SpError):
        sp.PolarGrid(1.0, 1.0, -1.0)
    with pytest.raises(sp.SpError):
        sp.PolarGrid(1.0, 1.0, 1.0, coord="radar")
    g = sp.PolarGrid(0.5, 0.25, 0.125, coord="lidar")
    assert (g.get_distance_voxel_size(), g.get_elevation_voxel_size(), g.get_azimuth_voxel_size()) == (0.5, 0.25, 0.125)
    g.set_coordinate_system("Camera")
    assert g.get_coordinate_system() == "CAMERA"
    with pytest.raises(sp.SpError):
        g.set_azimuth_voxel_size(0.0)
    assert sp.coordinate_system_from_string("LiDaR") == "LIDAR"
