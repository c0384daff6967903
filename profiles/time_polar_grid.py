"""PolarGrid against VoxelGrid (0.1 m) on the same clouds in one process: one JSON line.

Clouds: a synthetic spinning-LiDAR scan in its sensor frame (128 beams x 8192 azimuth steps = 1 048 576 points, ranges 1-80 m)
and the two bundled scans (tests/golden/source.ply, target.ply). Per cloud and grid: the median of 30 calls (after 5 of warm-up)
of the C-ABI call with the key box of the previous call known (sp_voxel_downsample_report / sp_polar_downsample_report, timed
by HIP events), its launches, and the median of 20 whole facade calls (VoxelGrid / PolarGrid.downsampling: key box protocol
and the voxel count read back). Run from the repository root: python profiles/time_polar_grid.py"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sycl_points_amd.api as sp  # noqa: E402
from sycl_points_amd import _lib  # noqa: E402

DEG = np.pi / 180.0


def spinning_scan(beams=128, steps=8192, seed=0):
    rs = np.random.RandomState(seed)
    el = np.linspace(-25.0 * DEG, 15.0 * DEG, beams)
    az = np.linspace(-np.pi, np.pi, steps, endpoint=False)
    E, A = np.meshgrid(el, az, indexing="ij")
    R = rs.uniform(1.0, 80.0, E.shape)
    R = np.where(E < -5 * DEG, np.minimum(R, 1.7 / np.maximum(np.sin(-E), 1e-3)), R)  # a floor 1.7 m below the sensor
    pts = np.ones((E.size, 4), np.float32)
    pts[:, 0] = (R * np.cos(E) * np.cos(A)).ravel()
    pts[:, 1] = (R * np.cos(E) * np.sin(A)).ravel()
    pts[:, 2] = (R * np.sin(E)).ravel()
    return pts


def read_ply_xyz(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int([ln for ln in head.split(b"\n") if ln.startswith(b"element vertex")][0].split()[-1])
    a = np.frombuffer(body, dtype="<f4", count=n * 4).reshape(n, 4)
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = a[:, :3]
    return pts


def median_ms(fn, runs=30, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t))


def wall_ms(fn, runs=20, warmup=3):
    import time
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def count_launches(fn):
    """kernels one call enqueues, from torch's profiler (HIP activity)"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def measure(P, grid, report_call):
    n = P.shape[0]
    L = _lib.lib()
    voxels = grid.downsampling(P).size()  # (remembers the key box)
    grid.downsampling(P)
    box = grid._key_box
    nbytes = L.sp_voxel_downsample_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=P.device)
    o_p = torch.empty((n, 4), dtype=torch.float32, device=P.device)
    info = torch.zeros(8, dtype=torch.int32, device=P.device)
    rest = (None, None, None, sp._ptr(o_p), None, None, None, None, None, box.ctypes.data_as(C.c_void_p), sp._ptr(info),
            sp._ptr(ws), nbytes, sp._stream())

    def run():
        _lib.check(report_call(sp._ptr(P), n, rest))

    ms = median_ms(run)
    assert int(info[0]) == voxels and int(info[1]) == 0
    return {"ms": ms, "voxels": voxels, "launches": count_launches(run), "ms_whole_api_call": wall_ms(lambda: grid.downsampling(P))}


def main():
    L = _lib.lib()
    torch.cuda.set_device(0)
    clouds = {"spinning_lidar_1M": spinning_scan()}
    for name in ("source.ply", "target.ply"):
        clouds[name] = read_ply_xyz(os.path.join(ROOT, "tests", "golden", name))
    polar_sizes = (0.5, 1.0 * DEG, 1.0 * DEG)
    out = {"polar_sizes": {"distance_m": polar_sizes[0], "elevation_deg": 1.0, "azimuth_deg": 1.0}, "voxel_size_m": 0.1,
           "timing": "median of 30 C-ABI calls after 5 warm-up (HIP events, key box known); whole facade call: median of 20"}
    for name, pts in clouds.items():
        P = torch.from_numpy(pts).cuda()
        vg = sp.VoxelGrid(0.1)
        v = measure(P, vg, lambda p, n, rest: L.sp_voxel_downsample_report(p, n, vg.voxel_size_inv, 1, *rest))
        row = {"points": int(len(pts)), "voxel_grid": v}
        for coord in ("LIDAR", "CAMERA"):
            pg = sp.PolarGrid(*polar_sizes, coord=coord)
            k = pg._key_args()
            row[f"polar_grid_{coord.lower()}"] = measure(
                P, pg, lambda p, n, rest, k=k: L.sp_polar_downsample_report(p, n, *k, 1, *rest))
        row["ratio_polar_lidar_to_voxel"] = row["polar_grid_lidar"]["ms"] / v["ms"]
        out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
