"""OccupancyGridMap::extract_visible_points on the GPU (sp_ogm_extract_visible_points, api.OccupancyGridMap and, through
tests/cpp/test_occupancy_visible.cpp, the C++ facade) against the CPU restatement (tests/cpp/occupancy_visible_restate.cpp, pinned
by tests/test_occupancy_visible_cpu.py, whose helpers are used here with those of the two occupancy-grid suites).

Centroid sums on the device are relaxed float atomics, so the restatement is always given the device's own export(), never the
restated map's. From identical bits every decision is identical: the visible keys must be EQUAL, and since both sides keep
table-slot order, equal as arrays. Rows are bit-identical to extract_occupied_points' rows for the same keys (one write_mean_row).
No ray here is longer than about 45 steps."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 4096)  # one lane | 63, 64, 65 candidates on the walk kernel: a wave and its edges | many workgroups
VOXEL = 0.5


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


@pytest.fixture(scope="module")
def vis():
    import importlib.util

    spec = importlib.util.spec_from_file_location("ogm_visible_cpu_helpers", os.path.join(ROOT, "tests", "test_occupancy_visible_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def cpu(vis):
    return vis.load_helpers("test_occupancy_grid_cpu.py", "ogm_cpu_helpers")


@pytest.fixture(scope="module")
def gpu(vis):
    return vis.load_helpers("test_gpu_occupancy_grid.py", "ogm_gpu_helpers")


@pytest.fixture(scope="module")
def V(vis, tmp_path_factory):
    return vis.build_visible_restatement(tmp_path_factory.mktemp("ogm_visible_gpu"))


def host(t):
    return None if t is None else t.cpu().numpy()


def visible_rows(m, pose, args):
    r = m.extract_visible_points(np.eye(4, dtype=np.float32) if pose is None else pose, *args)
    return {"points": host(r.points).reshape(-1, 4), "covs": host(r.covs) if r.has_cov() else None,
            "rgb": host(r.rgb) if r.has_rgb() else None, "intensities": host(r.intensities) if r.has_intensity() else None,
            "keys": host(r.keys).view(np.uint64), "size": r.size()}


def check_against_restatement(vis, V, m, pose, args):
    """the device's visible keys against the restatement on the device's own export; returns the rows and the restatement's counts"""
    e = m.export()
    got = visible_rows(m, pose, args)
    want, counts = vis.restated_visible(V, e, m.voxel_size(), 0.0, pose, *args)
    assert np.array_equal(got["keys"], want), (len(got["keys"]), len(want), counts)
    assert got["size"] == len(want) == len(got["points"]) and len(np.unique(got["keys"])) == len(got["keys"])
    return got, counts


def test_reference_known_answers_and_the_wall(sp, vis, gpu):
    def visible(dev, pose, d, hf, vf):
        occupied = dev.m.extract_occupied_points(pose, 1e6).size()
        return visible_rows(dev.m, pose, (d, hf, vf))["points"], occupied

    vis.known_answers(lambda voxel_size: gpu.DevMap(sp, voxel_size), lambda dev, pts: dev.add_point_cloud(pts), visible)


@pytest.fixture(scope="module")
def maps(sp, gpu):
    """api.OccupancyGridMap after the random cloud's first n points from POSE with every attribute, by (n, carving); built once
    and only read"""
    big = gpu.make_cloud(4096, seed=31)
    out = {}
    for n in SIZES:
        for carving in (False, True):
            dev = gpu.DevMap(sp, VOXEL)
            dev.set("free_space_updates_enabled", int(carving))
            dev.add_point_cloud(big["pts"][:n], gpu.POSE, big["covs"][:n], big["rgb"][:n], big["intensities"][:n])
            out[n, carving] = dev.m
    return out


@pytest.mark.parametrize("carving", (False, True), ids=("hits", "carved"))
@pytest.mark.parametrize("n", SIZES)
def test_visible_set_equals_the_restatement(vis, V, gpu, maps, n, carving):
    m = maps[n, carving]
    for name, args in vis.ARGS.items():
        got, (cand, occluded, longest) = check_against_restatement(vis, V, m, gpu.POSE, args)
        print(f"n = {n}, carving {carving}, {name}: {cand} candidates, {len(got['keys'])} visible, longest walk {longest} steps")
        assert longest <= 45
        if n == 4096 and name == "sphere":
            assert 0 < len(got["keys"]) < cand
        if name == "sphere" and not carving:
            assert cand == m.info("voxel_num")  # hits only: every voxel is occupied, and a candidate of the whole sphere


def test_rows_are_those_of_extract_occupied_points(vis, gpu, maps):
    for key in ((4096, False), (4096, True), (65, False)):
        m = maps[key]
        got = visible_rows(m, gpu.POSE, vis.ARGS["sphere"])
        r = m.extract_occupied_points(gpu.POSE, 1e6)
        all_keys = host(r.keys).view(np.uint64)
        order = np.argsort(all_keys)
        row = order[np.searchsorted(all_keys[order], got["keys"])]
        assert len(got["keys"]) > 0 and np.array_equal(all_keys[row], got["keys"])
        for name, full in (("points", r.points), ("covs", r.covs), ("rgb", r.rgb), ("intensities", r.intensities)):
            assert got[name] is not None
            a, b = got[name].reshape(len(row), -1), host(full).reshape(len(all_keys), -1)[row]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


def test_call_is_read_only_and_repeatable(vis, gpu, maps):
    m = maps[4096, True]
    before = m.export()
    first = visible_rows(m, gpu.POSE, vis.ARGS["frustum"])
    second = visible_rows(m, gpu.POSE, vis.ARGS["frustum"])
    after = m.export()
    for k in before:
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
    assert len(first["keys"]) > 0
    for k in ("keys", "points", "covs", "rgb", "intensities"):
        assert np.array_equal(first[k].view(np.uint8), second[k].view(np.uint8)), k


def test_tombstones(sp, vis, V, gpu, cpu):
    """stale_frame_threshold 2, carving off: 2048 points in frame 0, the other 2048 in frames 1 to 3. Where a voxel of the second
    half found its first slots taken by the first half it sits further along its probe sequence; the prune of frame 3 turns the
    first half's slots into `deleted` keys, and the probes of the walk have to step over them to find it."""
    big = gpu.make_cloud(4096, seed=31)["pts"]
    dev = gpu.DevMap(sp, VOXEL)
    dev.set("free_space_updates_enabled", 0)
    dev.set("stale_frame_threshold", 2)
    dev.add_point_cloud(big[:2048], gpu.POSE)
    first = dev.info("voxel_num")
    for _ in range(3):
        dev.add_point_cloud(big[2048:], gpu.POSE)
    kept = dev.info("voxel_num")
    assert 1000 < kept <= 2048 < first + kept - 200 and dev.info("capacity") == 30029  # most of the first half is pruned
    for args in vis.ARGS.values():
        got, (cand, _, _) = check_against_restatement(vis, V, dev.m, gpu.POSE, args)
        assert 0 < len(got["keys"]) <= cand


def test_after_growth(sp, vis, V, gpu, cpu):
    """rehash_threshold 0.01 as in test_export_scratch_regrows: one call on 30 029 slots, one on 60 013 of the same object — the
    scratch, candidate list included, has to grow with the table"""
    dev = gpu.DevMap(sp, VOXEL)
    dev.set("free_space_updates_enabled", 0)
    dev.set("rehash_threshold", 0.01)
    pose = vis.identity_at((-1.3, 2.1, 1.7))
    first = 0
    for frames, voxels, capacity in (((64,), 64, 30029), ((250, 150), 464, 60013)):
        for count in frames:
            k = np.arange(first, first + count)
            first += count
            dev.add_point_cloud(cpu.P((np.stack([k % 8, (k // 8) % 8, k // 64], axis=1) + 0.5) * VOXEL))
        assert (dev.info("voxel_num"), dev.info("capacity")) == (voxels, capacity)
        got, (cand, occluded, _) = check_against_restatement(vis, V, dev.m, pose, vis.SPHERE)
        assert cand == voxels and 0 < occluded < cand  # a solid block of cells: the outer ones hide the inner ones


def test_early_returns(sp, vis, gpu, cpu):
    m = sp.OccupancyGridMap(VOXEL)
    r = m.extract_visible_points(np.eye(4, dtype=np.float32), *vis.SPHERE)
    assert r.size() == 0 and len(r.keys) == 0
    m.add_point_cloud(gpu.dev_cloud(sp, cpu.P([[1.1, 0.1, 0.1], [2.1, 0.1, 0.1]])))
    assert m.extract_visible_points(np.eye(4, dtype=np.float32), *vis.SPHERE).size() == 1
    # out_capacity below voxel_num
    from sycl_points_amd import _lib
    import ctypes as C

    pts, n_out = torch.empty((8, 4), dtype=torch.float32, device="cuda"), C.c_size_t(0)
    pose = vis.T16(None)
    rc = _lib.lib().sp_ogm_extract_visible_points(m._h, pose.ctypes.data_as(C.c_void_p), 100.0, 1.0, 1.0, pts.data_ptr(), None, None,
                                                  None, None, m.info("voxel_num") - 1, C.byref(n_out), None)
    assert rc == 1 and b"extract_visible_points" in _lib.lib().sp_last_error()
    with pytest.raises(sp.SpError) as e:
        sp.check(rc)
    assert e.value.code == 1
    # a sensor outside the 21-bit cell range: nothing, and no device error
    assert m.extract_visible_points(vis.identity_at((1e7, 0, 0)), *vis.SPHERE).size() == 0
    torch.cuda.synchronize()
    for bad in ((100.0, float("nan"), 1.0), (100.0, 1.0, float("nan")), (float("nan"), 1.0, 1.0), (100.0, float("inf"), 1.0)):
        with pytest.raises(sp.SpError) as e:
            m.extract_visible_points(np.eye(4, dtype=np.float32), *bad)
        assert e.value.code == 1
    assert m.extract_visible_points(vis.identity_at((np.nan, 0, 0)), *vis.SPHERE).size() == 0  # a position without a cell
    bad_rotation = np.eye(4, dtype=np.float32)
    bad_rotation[1, 1] = np.inf
    with pytest.raises(sp.SpError) as e:
        m.extract_visible_points(bad_rotation, *vis.SPHERE)
    assert e.value.code == 1
    assert m.extract_visible_points(np.eye(4, dtype=np.float32), float("inf"), 1.0, 1.0).size() == 1  # +inf: no distance bound
    torch.cuda.synchronize()


def test_cpp_facade(sp):
    """tests/cpp/test_occupancy_visible.cpp, built with tests/cpp/Makefile's flags and libraries (the Makefile is not changed): the
    reference's three cases and the wall through sycl_points::algorithms::mapping::OccupancyGridMap"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(cpp, "test_occupancy_visible")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    lib = os.path.join(ROOT, "sycl_points_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++20", f"-I{ROOT}/include", f"-I{rocm}/include", "-D__HIP_PLATFORM_AMD__", "-Wall",
                           "-Wno-unused-value", "-Wno-unused-result", os.path.join(cpp, "test_occupancy_visible.cpp"), "-o", exe,
                           f"-L{lib}", "-lsycl_points_amd", f"-Wl,-rpath,{lib}", f"-L{rocm}/lib", "-lamdhip64",
                           f"-Wl,-rpath,{rocm}/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failed" in r.stdout
