"""PointCloud2 ingestion on the device (sp_pc2_unpack, sp_pc2_pack, sp_enhanced_reflectivity; api.from_pointcloud2 /
to_pointcloud2 / EnhancedReflectivityCorrector; through tests/cpp/test_ros2_convert.cpp the C++ facade's ros2::fromROS2msg /
toROS2msg / EnhancedReflectivityCorrector) against the numpy restatement of tests/test_pointcloud2_cpu.py.

Unpack and pack are bit-exact: every arithmetic step is one correctly rounded IEEE operation, so there is no tolerance (if
`/ 255.0f` were not bit-exact the build flags changed: fix those). The reflectivity correction is bit-exact on inputs whose sums
are exact in any order, and on random inputs it is held to (c_max + 16 + 3 s) * 2^-24 relative to a float64 evaluation (derived in
tests/test_pointcloud2_cpu.py, where the sequential float32 restatement is shown to satisfy it with room to spare). Every figure
is printed before it is asserted (run with -s). Measured on an MI355X: unpack and pack bit-exact on every layout and size; the
reflectivity's largest relative error 2.7e-7 against bounds of 3.16e-5 to 3.20e-5 (c_max 510 to 512, 1 to 3 scans), the same for the
one-byte and the two-byte ring field.
"""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
SENTINEL = -123.25


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


@pytest.fixture(scope="module")
def cpu():
    spec = importlib.util.spec_from_file_location("pointcloud2_cpu_helpers", os.path.join(ROOT, "tests", "test_pointcloud2_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: frombuffer's arrays are read-only)


def unpack_raw(data_dev, nbytes, n, layout, n_alloc):
    """sp_pc2_unpack into tensors of n_alloc rows pre-filled with a sentinel, every attribute allocated whether the layout has it
    or not: numpy (points, rgb, intensities, timestamps, max)"""
    from sycl_points_amd import _lib

    L = _lib.lib()
    f = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")  # noqa: E731
    P, R, I, T = f(n_alloc, 4), f(n_alloc, 4), f(n_alloc), f(n_alloc)
    M = torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda")
    W = torch.empty(max(L.sp_pc2_unpack_workspace_bytes(n), 16), dtype=torch.uint8, device="cuda")
    rc = L.sp_pc2_unpack(_vp(data_dev.data_ptr()), nbytes, n, C.byref(layout), *[_vp(x.data_ptr()) for x in (P, R, I, T, M, W)],
                         _vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.sp_last_error()
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (P, R, I, T, M))


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_unpack_is_bit_exact(sp, cpu, name):
    step, fields = cpu.LAYOUTS[name]
    n_max = cpu.SIZES[-1]
    data = cpu.make_message(name, n_max).tobytes()
    rc, layout = cpu.resolve(fields, step)
    assert rc == 0
    layout.start_time_ms = cpu.START_MS
    data_dev = dev(np.frombuffer(data, np.uint8))
    for n in cpu.SIZES:
        ref = cpu.restate_unpack(data, n, layout)
        # data_bytes = n * point_step: the kernel is told the buffer ends with its last record
        out = unpack_raw(data_dev, n * step, n, layout, n_max + 5)
        for k, (o, r) in enumerate(zip(out[:4], ref[:4])):
            what = ("points", "rgb", "intensities", "timestamps")[k]
            if r is None:
                assert np.all(o == np.float32(SENTINEL)), (name, n, what, "absent attribute written")
                continue
            assert np.array_equal(bits(o[:n]), bits(r)), (name, n, what, np.flatnonzero((bits(o[:n]) != bits(r)).reshape(n, -1).any(1))[:8])
            assert np.all(o[n:] == np.float32(SENTINEL)), (name, n, what, "rows >= n written")
        if ref[4] is None:
            assert out[4][0] == SENTINEL
        else:
            print(f"unpack [{name} n = {n}] max offset: device {out[4][0]!r}, restatement {ref[4]!r}")
            assert bits(out[4])[0] == bits(np.float64([ref[4]]))[0], (name, n)


def test_from_pointcloud2_mirror(sp, cpu):
    n = cpu.SIZES[-1]
    for name in ("a", "c", "d"):
        step, fields = cpu.LAYOUTS[name]
        data = cpu.make_message(name, n).tobytes()
        layout = cpu.resolve(fields, step)[1]
        layout.start_time_ms = cpu.START_MS
        ref = cpu.restate_unpack(data, n, layout)
        buf = dev(np.frombuffer(data, np.uint8))
        cloud = sp.from_pointcloud2(buf, fields, step, cpu.STAMP)
        for t, r in zip((cloud.points, cloud.rgb, cloud.intensities, cloud.timestamp_offsets), ref[:4]):
            assert (t is None) == (r is None)
            if r is not None:
                assert np.array_equal(bits(t.cpu().numpy()), bits(r))
        if ref[4] is None:
            assert (cloud.start_time_ms, cloud.end_time_ms) == (0.0, 0.0)
        else:
            assert (cloud.start_time_ms, cloud.end_time_ms) == (cpu.START_MS, cpu.START_MS + ref[4])
    step, fields = cpu.LAYOUTS["a"]
    off = sp.from_pointcloud2(buf := dev(np.frombuffer(cpu.make_message("a", 70).tobytes(), np.uint8)), fields, step, cpu.STAMP,
                              convert_intensity=False)
    assert off.intensities is None and off.size() == 70
    assert sp.from_pointcloud2(buf, fields, step, cpu.STAMP, is_bigendian=True) is None
    assert sp.from_pointcloud2(buf, fields[1:], step, cpu.STAMP) is None  # no x
    assert sp.from_pointcloud2(buf[:0], fields, step, cpu.STAMP).size() == 0


ATTRS = {"points": (False, False, False), "rgb": (True, False, False), "intensity+time": (False, True, True), "all": (True, True, True)}
RGB_SPECIALS = (-0.5, 0.0, 0.999, 1.0, 1.5, np.nan, 1.0 / 255.0, 0.5)


def pack_inputs(cpu, n):
    rs = np.random.RandomState(5)
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = rs.uniform(-50, 50, (n, 3))
    pts[0, :3] = (np.nan, np.inf, -0.0)
    rgb = rs.uniform(-0.2, 1.2, (n, 4)).astype(np.float32)
    k = min(len(RGB_SPECIALS), rgb.size)
    rgb.reshape(-1)[:k] = RGB_SPECIALS[:k]
    inten = rs.uniform(0, 300, n).astype(np.float32)
    ts = rs.uniform(0, 100, n).astype(np.float32)
    return pts, rgb, inten, ts


@pytest.mark.parametrize("attrs", list(ATTRS))
def test_pack_is_bit_exact(sp, cpu, attrs):
    """NaN in rgb packs to 0: clamp is fminf(fmaxf(c, 0), 1), fmaxf(NaN, 0) = 0 — pinned in the restatement's own test"""
    has_rgb, has_int, has_ts = ATTRS[attrs]
    for n in (1, cpu.B - 1, cpu.B, cpu.SIZES[-1]):
        pts, rgb, inten, ts = pack_inputs(cpu, n)
        cloud = sp.PointCloudShared.from_numpy(pts, rgb=rgb if has_rgb else None, intensities=inten if has_int else None,
                                               timestamp_offsets=ts if has_ts else None)
        cloud.start_time_ms = cpu.START_MS
        data, fields, step = sp.to_pointcloud2(cloud)
        ref = cpu.restate_pack(pts, rgb if has_rgb else None, inten if has_int else None, ts if has_ts else None, cpu.START_MS)
        got = data.cpu().numpy().tobytes()
        assert step == len(ref) // n and len(got) == len(ref)
        assert got == ref, (attrs, n, np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(ref, np.uint8))[:8])
        assert [f[0] for f in fields] == ["x", "y", "z"] + [k for k, h in (("rgb", has_rgb), ("intensity", has_int), ("timestamp", has_ts)) if h]
        dt = cpu.pack_dtype(has_rgb, has_int, has_ts)
        for name, offset, _, count in fields[3:]:  # the declared offsets are where the data is
            assert offset == dt.fields[name][1] and count == 1


def test_round_trip(sp, cpu):
    n = cpu.SIZES[-1]
    pts, rgb, inten, ts = pack_inputs(cpu, n)
    pts[0, :3] = (1.0, 2.0, 3.0)
    rgb = np.nan_to_num(rgb)
    cloud = sp.PointCloudShared.from_numpy(pts, rgb=rgb, intensities=inten, timestamp_offsets=ts)
    cloud.start_time_ms = cpu.START_MS
    data, fields, step = sp.to_pointcloud2(cloud)
    back = sp.from_pointcloud2(data, [f[:3] for f in fields], step, cpu.STAMP)
    assert np.array_equal(bits(back.points.cpu().numpy()), bits(pts))
    assert np.array_equal(bits(back.intensities.cpu().numpy()), bits(inten))
    q = (np.clip(rgb, 0, 1) * np.float32(255)).astype(np.uint8).astype(np.float32) / np.float32(255)
    assert np.array_equal(bits(back.rgb.cpu().numpy()), bits(q))
    # the time stamps went through seconds as doubles: 1.7e12 ms resolves 2.4e-4 ms
    assert np.abs(back.timestamp_offsets.cpu().numpy().astype(np.float64) - ts).max() < 1e-3
    assert back.start_time_ms == cpu.START_MS


def er_run(sp, cpu, kind, scans, alpha, clip, shared_corrector=None):
    """the scans through api.from_pointcloud2 + EnhancedReflectivityCorrector.apply: per scan (intensities, state) as numpy"""
    step, fields = cpu.ER_LAYOUTS[kind]
    corr = shared_corrector or sp.EnhancedReflectivityCorrector(alpha)
    out = []
    for pts, inten, ring, amb in scans:
        buf = dev(np.frombuffer(cpu.reflectivity_message(kind, pts, inten, ring, amb).tobytes(), np.uint8))
        cloud = sp.from_pointcloud2(buf, fields, step, cpu.STAMP, use_reflectivity_as_intensity=False)
        assert np.array_equal(bits(cloud.intensities.cpu().numpy()), bits(inten))
        assert corr.apply(cloud, buf, fields, step, clip) is True
        st = corr.state.cpu().numpy()
        out.append((cloud.intensities.cpu().numpy(), [st[:256].view(np.float32), st[256:512].view(np.float32), st[512:] != 0]))
    return out


def test_reflectivity_exact_case(sp, cpu):
    """every operation exact in any order: output and state bit-identical to the sequential restatement after each of three
    scans; the third leaves ring 5 absent (its means stay)"""
    scans = [cpu.exact_scan(s) for s in range(3)]
    got = er_run(sp, cpu, "u16", scans, 0.5, 5.0)
    state = cpu.new_state()
    for s, (scan, (inten_dev, state_dev)) in enumerate(zip(scans, got)):
        before = [x.copy() for x in state]
        ref, _, count = cpu.restate_reflectivity(*scan, state, 0.5, 5.0)
        assert count.max() <= 512
        assert np.array_equal(bits(inten_dev), bits(ref)), (s, np.flatnonzero(bits(inten_dev) != bits(ref))[:8])
        assert np.array_equal(bits(state_dev[0]), bits(state[0])) and np.array_equal(bits(state_dev[1]), bits(state[1]))
        assert np.array_equal(state_dev[2], state[2])
        if s == 2:
            assert count[5] == 0 and state[0][5] == before[0][5] != 0
    assert (got[0][0] == 5.0).any() and (got[0][0] == 0.0).any()


@pytest.mark.parametrize("kind", ["u16", "u8"])
def test_reflectivity_general_case(sp, cpu, kind):
    scans = [cpu.general_scan(kind, s) for s in range(3)]
    got = er_run(sp, cpu, kind, scans, 0.5, 1e30)  # (nothing clamps: the bound is on the value before clamping)
    again = er_run(sp, cpu, kind, scans, 0.5, 1e30)
    s64 = cpu.new_state(np.float64)
    for s, (scan, (inten_dev, state_dev)) in enumerate(zip(scans, got)):
        _, raw64, count = cpu.restate_reflectivity(*scan, s64, 0.5, 1e30, np.float64)
        bound = cpu.reflectivity_bound(int(count.max()), s + 1)
        pos = raw64 > 0
        rel = np.abs(inten_dev.astype(np.float64) - raw64)[pos] / raw64[pos]
        print(f"reflectivity [{kind} scan {s}] max relative error {rel.max():.3e}, bound {bound:.3e}, c_max {count.max()}")
        assert np.array_equal(inten_dev == 0, ~pos)  # rings >= 256 and points at the sensor give 0, nothing else does
        assert rel.max() <= bound
        srel = np.abs(state_dev[0][:17].astype(np.float64) - s64[0][:17]) / np.maximum(s64[0][:17], 1e-300)
        assert srel.max() <= bound and np.array_equal(state_dev[2], s64[2])
        assert np.array_equal(bits(inten_dev), bits(again[s][0]))  # two runs: identical bits
        for x, y in zip(state_dev, again[s][1]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_reflectivity_refuses_a_message_without_ambient(sp, cpu):
    step, fields = cpu.ER_LAYOUTS["u16"]
    pts, inten, ring, amb = cpu.general_scan("u16", 0)
    buf = dev(np.frombuffer(cpu.reflectivity_message("u16", pts, inten, ring, amb).tobytes(), np.uint8))
    cloud = sp.from_pointcloud2(buf, fields, step, cpu.STAMP, use_reflectivity_as_intensity=False)
    corr = sp.EnhancedReflectivityCorrector()
    assert corr.apply(cloud, buf, [f for f in fields if f[0] != "ambient"], step) is False
    assert corr.apply(cloud, buf, [(f[0], f[1], cpu.F32 if f[0] == "ring" else f[2]) for f in fields], step) is False
    assert np.array_equal(bits(cloud.intensities.cpu().numpy()), bits(inten)) and corr.state is None
    cloud.intensities = None
    assert corr.apply(cloud, buf, fields, step) is False


def test_cpp_facade(sp):
    """tests/cpp/test_ros2_convert.cpp, built with tests/cpp/Makefile's flags and libraries (the Makefile is not changed): the
    fromROS2msg overloads, a larger msg_buffer reused, the empty and the big-endian message, toROS2msg's offsets, apply with and
    without the shared buffer, and a converted scan through LiDAROdometryPipeline::process."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(cpp, "test_ros2_convert")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    lib = os.path.join(ROOT, "sycl_points_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++20", f"-I{ROOT}/include", f"-I{rocm}/include", "-D__HIP_PLATFORM_AMD__", "-Wall",
                           "-Wno-unused-value", "-Wno-unused-result", os.path.join(cpp, "test_ros2_convert.cpp"), "-o", exe,
                           f"-L{lib}", "-lsycl_points_amd", f"-Wl,-rpath,{lib}", f"-L{rocm}/lib", "-lamdhip64",
                           f"-Wl,-rpath,{rocm}/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failed" in r.stdout
