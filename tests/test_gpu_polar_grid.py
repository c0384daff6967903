"""PolarGrid on the device (sp_polar_keys, sp_polar_key_box, sp_polar_downsample_report, the Python and C++ facades) against
the host twin of its key (sp_polar_keys_host) and a CPU restatement of the reference's aggregation
(filter/polar_downsampling.hpp:316-440): stable order of the keys, float32 sums in ascending point index, mean = sum / count,
median of intensities with 0.5f * (lower + upper) for an even count."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
DEG = np.pi / 180.0


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def inv(v):
    return float(np.float32(1.0) / np.float32(v))


def host_keys(sp, pts, coord, d, e, a):
    L = sp._lib.lib()
    pts = np.ascontiguousarray(pts, np.float32)
    keys = np.empty(len(pts), np.uint64)
    sp._lib.check(L.sp_polar_keys_host(pts.ctypes.data_as(C.c_void_p), len(pts), sp._lib.COORD[coord], inv(d), inv(e), inv(a),
                                       keys.ctypes.data_as(C.c_void_p)))
    return keys


def restate(keys, pts, minc, rgb=None, inten=None, ts=None):
    """The reference's aggregation over the host twin's keys, in float32, points summed in ascending index order."""
    idx = np.flatnonzero(keys != INVALID)
    order = idx[np.argsort(keys[idx], kind="stable")]
    k = keys[order]
    out = {"keys": k[:0], "points": np.zeros((0, 4), np.float32), "rgb": np.zeros((0, 4), np.float32),
           "intensities": np.zeros(0, np.float32), "timestamps": np.zeros(0, np.float32)}
    if len(k) == 0:
        return out
    starts = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
    lens = np.diff(np.r_[starts, len(k)])

    def sums(vals):  # position j of every run long enough, added into that run's accumulator: index order, vectorised
        acc = np.zeros((len(starts),) + vals.shape[1:], np.float32)
        for j in range(int(lens.max())):
            live = lens > j
            acc[live] = acc[live] + vals[order[starts[live] + j]]
        return acc

    ps = sums(pts.astype(np.float32))
    w = ps[:, 3]
    keep = w >= np.float32(minc)
    out["keys"] = k[starts][keep]
    out["points"] = (ps / w[:, None])[keep]
    if rgb is not None:
        out["rgb"] = (sums(rgb) / w[:, None])[keep]
    if ts is not None:
        out["timestamps"] = (sums(ts) / w)[keep]
    if inten is not None:
        run_id = np.repeat(np.arange(len(starts)), lens)
        v = inten[order]
        sv = v[np.lexsort((v, run_id))]
        mid = starts + lens // 2
        upper = sv[mid]
        lower = sv[np.maximum(mid - 1, starts)]
        med = np.where(lens % 2 == 1, upper, np.float32(0.5) * (lower + upper)).astype(np.float32)
        out["intensities"] = med[keep]
    return out


def spinning_scan(rs, beams=64, steps=2048, rmin=1.0, rmax=80.0):
    """A spinning LiDAR in its own frame: beams x azimuth steps, ranges rmin..rmax (a few walls and a floor)."""
    el = np.linspace(-25.0 * DEG, 15.0 * DEG, beams)
    az = np.linspace(-np.pi, np.pi, steps, endpoint=False)
    E, A = np.meshgrid(el, az, indexing="ij")
    R = rs.uniform(rmin, rmax, E.shape)
    R = np.where(E < -5 * DEG, np.minimum(R, 1.7 / np.maximum(np.sin(-E), 1e-3)), R)  # the floor 1.7 m below
    pts = np.ones((E.size, 4), np.float32)
    pts[:, 0] = (R * np.cos(E) * np.cos(A)).ravel()
    pts[:, 1] = (R * np.cos(E) * np.sin(A)).ravel()
    pts[:, 2] = (R * np.sin(E)).ravel()
    return pts


def edge_points():
    big = np.float32(3e38)
    return np.array([[np.nan, 1, 1, 1], [1, np.inf, 1, 1], [1, 1, -np.inf, 1], [0, 0, 0, 1], [-0.0, 0, -0.0, 1],
                     [0, 0, 5, 1], [0, 5, 0, 1], [0, -3, -0.0, 1], [1e-30, 1e-30, 1e-30, 1], [big, 1, 1, 1], [3e6, 0, 1, 1],
                     [-0.0, 2.0, 1.0, 1], [-3.0, -0.0, 1.0, 1], [-3.0, 0.0, -1.0, 1], [1e-38, -1e-38, 1e-38, 1]], np.float32)


def check_equal(out, keys, o):
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), o["keys"])
    assert np.array_equal(out.points.cpu().numpy().view(np.uint32), o["points"].view(np.uint32))
    if out.rgb is not None:
        assert np.array_equal(out.rgb.cpu().numpy(), o["rgb"])
    if out.intensities is not None:
        assert np.array_equal(out.intensities.cpu().numpy(), o["intensities"])
    if out.timestamp_offsets is not None:
        assert np.array_equal(out.timestamp_offsets.cpu().numpy(), o["timestamps"])


@pytest.mark.parametrize("coord", ["LIDAR", "CAMERA"])
def test_device_keys_equal_host_twin_bitwise(sp, coord):
    rs = np.random.RandomState(1)
    n = 1 << 20
    pts = np.ones((n, 4), np.float32)
    pts[: n // 2] = spinning_scan(rs, 64, n // 128)
    pts[n // 2:, :3] = (rs.standard_normal((n - n // 2, 3)) * np.float32(10.0) ** rs.uniform(-6, 6, (n - n // 2, 1))).astype(np.float32)
    e = edge_points()
    pts[: len(e)] = e
    for d, el, az in ((0.5, 1.0 * DEG, 1.0 * DEG), (0.1, 0.01, 0.003), (1.0, np.pi, np.pi), (1e-3, 1e-5, 1e-5)):
        g = sp.PolarGrid(d, el, az, coord=coord)
        k_dev = g.compute_polar_bit(dev(pts)).cpu().numpy().view(np.uint64)
        k_host = host_keys(sp, pts, coord, d, el, az)
        assert np.array_equal(k_dev, k_host), (d, el, az, np.flatnonzero(k_dev != k_host)[:8])
    assert (k_host[:11] == INVALID).sum() >= 9
    assert g.compute_polar_bit(dev(pts[:0])).numel() == 0


@pytest.mark.parametrize("coord", ["LIDAR", "CAMERA"])
@pytest.mark.parametrize("minc", [1, 2, 5])
def test_downsampling_equals_restatement(sp, coord, minc):
    rs = np.random.RandomState(10 + minc)
    pts = spinning_scan(rs, 32, 1024)
    e = edge_points()
    pts[: len(e)] = e
    n = len(pts)
    rgb = rs.uniform(0, 1, (n, 4)).astype(np.float32)
    inten = np.round(rs.uniform(0, 50, n)).astype(np.float32)  # ties
    ts = rs.uniform(0, 100, n).astype(np.float32)
    size = (0.5, 1.0 * DEG, 2.0 * DEG)
    keys = host_keys(sp, pts, coord, *size)
    g = sp.PolarGrid(*size, coord=coord)
    g.set_min_voxel_count(minc)
    pc = sp.PointCloudShared(dev(pts), rgb=dev(rgb), intensities=dev(inten), timestamp_offsets=dev(ts))
    o = restate(keys, pts, minc, rgb, inten, ts)
    assert len(o["keys"]) > 100
    for _ in range(2):  # the key box computed first, then the remembered one
        out, k = g.downsampling(pc, return_keys=True)
        check_equal(out, k, o)
    out = g.downsampling(sp.PointCloudShared(dev(pts)))  # points only
    assert np.array_equal(out.points.cpu().numpy(), o["points"]) and out.rgb is None and out.intensities is None


@pytest.mark.parametrize("coord", ["LIDAR", "CAMERA"])
def test_one_point_voxels_and_runs_of_thousands(sp, coord):
    rs = np.random.RandomState(3)
    n = 40000
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = rs.uniform(-30, 30, (n, 3))                                      # mostly one-point voxels at this size
    pts[10000:13000, :3] = np.float32([10.0, 10.0, 10.0]) + rs.uniform(-1e-3, 1e-3, (3000, 3)).astype(np.float32)
    pts[20000:24500, :3] = np.float32([-5.0, 7.0, 2.0])                           # 4500 identical points
    rgb = rs.uniform(0, 1, (n, 4)).astype(np.float32)
    inten = np.round(rs.uniform(0, 9, n)).astype(np.float32)
    ts = rs.uniform(0, 10, n).astype(np.float32)
    size = (0.05, 0.002, 0.002)
    keys = host_keys(sp, pts, coord, *size)
    o = restate(keys, pts, 1, rgb, inten, ts)
    _, cnt = np.unique(keys[keys != INVALID], return_counts=True)
    assert cnt.max() >= 3000 and (cnt == 1).sum() > 20000
    out, k = sp.PolarGrid(*size, coord=coord).downsampling(
        sp.PointCloudShared(dev(pts), rgb=dev(rgb), intensities=dev(inten), timestamp_offsets=dev(ts)), return_keys=True)
    check_equal(out, k, o)


def test_empty_and_all_invalid(sp):
    g = sp.PolarGrid(1.0, 0.1, 0.1)
    assert g.downsampling(dev(np.zeros((0, 4), np.float32))).size() == 0
    bad = edge_points()[:11]
    bad = bad[host_keys(sp, bad, "LIDAR", 1.0, 0.1, 0.1) == INVALID]
    out, k = g.downsampling(sp.PointCloudShared(dev(bad), intensities=dev(np.ones(len(bad), np.float32))), return_keys=True)
    assert out.size() == 0 and k.numel() == 0
    with pytest.raises(sp.SpError):
        sp.PolarGrid(1.0, 0.0, 1.0)


def test_reference_known_answer(sp):
    # test_downsampling_filters.cpp:90-136: two groups in the distance bins [1, 2) and [2, 3)
    pts = np.array([[1.10, 0, 0, 1], [1.40, 0, 0, 1], [2.10, 0, 0, 1], [2.30, 0, 0, 1], [2.40, 0, 0, 1]], np.float32)
    inten = np.array([2.0, 4.0, 6.0, 10.0, 100.0], np.float32)
    g = sp.PolarGrid(1.0, 3.14159265, 3.14159265, coord="LIDAR")
    g.set_min_voxel_count(2)
    out = g.downsampling(sp.PointCloudShared(dev(pts), intensities=dev(inten)))
    p, i = out.points.cpu().numpy(), out.intensities.cpu().numpy()
    assert p.shape[0] == 2
    assert abs(p[0, 0] - 1.25) < 1e-5 and abs(i[0] - 3.0) < 1e-5
    assert abs(p[1, 0] - 2.2666667) < 1e-5 and abs(i[1] - 10.0) < 1e-5


def test_boxed_path_equals_63bit_path_and_redo(sp):
    rs = np.random.RandomState(5)
    pts = spinning_scan(rs, 32, 1024, 1.0, 30.0)
    inten = rs.uniform(0, 255, len(pts)).astype(np.float32)
    size = (0.3, 0.5 * DEG, 0.5 * DEG)
    g = sp.PolarGrid(*size)
    pc = sp.PointCloudShared(dev(pts), intensities=dev(inten))
    b, kb = g.downsampling(pc, return_keys=True, boxed=False)
    for _ in range(2):
        a, ka = g.downsampling(pc, return_keys=True, boxed=True)
        assert torch.equal(ka, kb) and torch.equal(a.points, b.points) and torch.equal(a.intensities, b.intensities)
    check_equal(a, ka, restate(host_keys(sp, pts, "LIDAR", *size), pts, 1, inten=inten))
    # a second scan far outside the remembered box (ranges 100-200 m): redone with its own box, still the restatement
    far = spinning_scan(rs, 32, 1024, 100.0, 200.0)
    c, kc = g.downsampling(sp.PointCloudShared(dev(far), intensities=dev(inten)), return_keys=True, boxed=True)
    check_equal(c, kc, restate(host_keys(sp, far, "LIDAR", *size), far, 1, inten=inten))
    # the key box of the polar fields (sp_polar_key_box) is the min / max of the host twin's fields
    L = sp._lib.lib()
    box = torch.empty(6, dtype=torch.int32, device="cuda")
    P = dev(pts)
    sp._lib.check(L.sp_polar_key_box(sp._ptr(P), len(pts), 0, inv(size[0]), inv(size[1]), inv(size[2]), sp._ptr(box), sp._stream()))
    k = host_keys(sp, pts, "LIDAR", *size)
    k = k[k != INVALID]
    f = [(k >> np.uint64(s)) & np.uint64((1 << 21) - 1) for s in (0, 21, 42)]
    assert box.cpu().numpy().tolist() == [int(x.min()) for x in f] + [int(x.max()) for x in f]
    # changing a size forgets the box; the result follows the new size
    g.set_azimuth_voxel_size(2.0 * DEG)
    d, kd = g.downsampling(pc, return_keys=True)
    check_equal(d, kd, restate(host_keys(sp, pts, "LIDAR", size[0], size[1], 2.0 * DEG), pts, 1, inten=inten))


def read_ply_xyz(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int([ln for ln in head.split(b"\n") if ln.startswith(b"element vertex")][0].split()[-1])
    a = np.frombuffer(body, dtype="<f4", count=n * 4).reshape(n, 4)
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = a[:, :3]
    return pts


@pytest.mark.parametrize("name", ["source.ply", "target.ply"])
def test_bundled_scans(sp, name):
    pts = read_ply_xyz(os.path.join(GOLD, name))
    flags = sp.box_filter_flags(dev(pts), 1.0, 50.0)
    kept = sp.compact_by_flags(dev(pts), flags).cpu().numpy()
    assert 1000 < len(kept) < len(pts)
    for coord in ("LIDAR", "CAMERA"):
        size = (0.5, 1.0 * DEG, 1.0 * DEG)
        out, k = sp.PolarGrid(*size, coord=coord).downsampling(dev(kept), return_keys=True)
        o = restate(host_keys(sp, kept, coord, *size), kept, 1)
        check_equal(out, k, o)
        assert len(o["keys"]) < len(kept)


def test_knn_on_the_output_equals_bruteforce(sp):
    rs = np.random.RandomState(8)
    pts = spinning_scan(rs, 32, 1024, 1.0, 40.0)
    out = sp.PolarGrid(0.5, 0.5 * DEG, 0.5 * DEG).downsampling(dev(pts))
    tgt = out.points.contiguous()
    q = pts[::97].copy()
    q[:, :3] += rs.uniform(-0.05, 0.05, (len(q), 3)).astype(np.float32)  # (off the scan's symmetric lattice: no tied distances)
    qry = dev(q)
    for k in (1, 5, 10):
        bf = sp.knn_search_bruteforce(qry, tgt, k)
        for knn in (sp.KDTree.build(tgt), sp.GridKNN.build(tgt)):
            r = knn.knn_search(qry, k)
            assert torch.equal(r.indices, bf.indices) and torch.equal(r.distances, bf.distances)


def test_cpp_facade(sp):
    """tests/cpp/test_polar_grid.cpp, built with tests/cpp/Makefile's flags and libraries (the Makefile is not changed)."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(cpp, "test_polar_grid")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    lib = os.path.join(ROOT, "sycl_points_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++20", f"-I{ROOT}/include", f"-I{rocm}/include", "-D__HIP_PLATFORM_AMD__", "-Wall",
                           "-Wno-unused-value", "-Wno-unused-result", os.path.join(cpp, "test_polar_grid.cpp"), "-o", exe,
                           f"-L{lib}", "-lsycl_points_amd", f"-Wl,-rpath,{lib}", f"-L{rocm}/lib", "-lamdhip64",
                           f"-Wl,-rpath,{rocm}/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
