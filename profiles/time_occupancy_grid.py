"""OccupancyGridMap on the bundled scan (tests/golden/target.ply, 69 088 points, sensor at the origin) at voxel 0.25 m and 1.0 m:
add_point_cloud with carving off and on, and extract_occupied_points. HIP-event medians of 20 calls after 5 of warm-up, for the
first frame into a cleared map (the clear outside the events; with carving this includes the growth rehash) and for the same scan
added again to the grown map (the steady state of a submap). Also the voxel count, capacity and misses per ray. One JSON line.
A second JSON line for extract_visible_points on the carved 0.25 m map, from the scan's own sensor pose: its time beside
extract_occupied_points' (the same table pass and compaction without the walk; 3 warm-ups, 20 calls each), and for a 90 x 30 degree
frustum and the whole sphere the candidates, the visible voxels and the mean and largest number of walk steps per candidate (the
candidates and their step counts from a float32 numpy evaluation of the frustum test on export())."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sycl_points_amd.api as sp  # noqa: E402


def read_ply_xyz(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int([ln for ln in head.split(b"\n") if ln.startswith(b"element vertex")][0].split()[-1])
    a = np.frombuffer(body, dtype="<f4", count=n * 4).reshape(n, 4)
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = a[:, :3]
    return pts


def median_ms(fn, before=None, runs=20, warmup=5):
    t = []
    for i in range(warmup + runs):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            t.append(a.elapsed_time(b))
    return round(float(np.median(t)), 4)


def candidate_steps(e, voxel, pose, max_distance, horizontal_fov, vertical_fov):
    """walk steps (|dix| + |diy| + |diz| from the sensor's cell) of every candidate of extract_visible_points, from an export()"""
    f32, pi, tol = np.float32, np.float32(3.1415927), np.float32(1e-6)
    hf, vf = min(max(f32(horizontal_fov), tol), pi - tol), min(max(f32(vertical_fov), tol), f32(2) * pi - tol)
    seen = (e["hit_count"] > 0) & ~(e["log_odds"] < 0)
    cen = e["sum_xyz"][seen] * (f32(1) / e["hit_count"][seen].astype(f32))[:, None]
    d = cen - pose[:3, 3]
    local = d @ pose[:3, :3]  # R^T d
    forward = np.abs(local[:, 0]) if hf >= pi - tol else local[:, 0]
    keep = ((d * d).sum(axis=1) <= f32(max_distance) ** 2) & (forward > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for side, fov in ((local[:, 1], hf), (local[:, 2], vf)):
            keep &= ~(forward / np.sqrt(forward * forward + side * side) < np.cos(fov * f32(0.5)))
    inv = f32(1) / f32(voxel)
    return np.abs(np.floor(cen[keep] * inv) - np.floor(pose[:3, 3] * inv)).sum(axis=1)


cloud = sp.PointCloudShared(torch.from_numpy(read_ply_xyz(os.path.join(ROOT, "tests", "golden", "target.ply"))).cuda())
out = {"points": cloud.size()}
for voxel in (0.25, 1.0):
    for carving in (False, True):
        m = sp.OccupancyGridMap(voxel)
        m.set_free_space_updates_enabled(carving)
        tag = f"voxel_{voxel}_carving_{'on' if carving else 'off'}"
        out[f"{tag}_first_frame_ms"] = median_ms(lambda: m.add_point_cloud(cloud), before=m.clear)
        m.clear()
        m.add_point_cloud(cloud)
        out[f"{tag}_steady_frame_ms"] = median_ms(lambda: m.add_point_cloud(cloud))
        out[f"{tag}_extract_ms"] = median_ms(lambda: m.extract_occupied_points(max_distance=100.0))
        e = m.export()
        out[f"{tag}_voxels"], out[f"{tag}_capacity"] = m.info("voxel_num"), m.info("capacity")
        out[f"{tag}_occupied"] = m.extract_occupied_points(max_distance=100.0).size()
        out[f"{tag}_misses_per_ray_per_frame"] = round(float(e["miss_count"].sum()) / m.info("frame_index") / cloud.size(), 2)
        if voxel == 0.25 and carving:
            pose = np.eye(4, dtype=np.float32)
            vis = {"map": tag, "voxels": m.info("voxel_num"), "capacity": m.info("capacity"),
                   "extract_occupied_ms": median_ms(lambda: m.extract_occupied_points(pose, 100.0), warmup=3)}
            for name, (hf, vf) in (("frustum_90x30", (np.pi / 2, np.pi / 6)), ("sphere", (np.pi, 2 * np.pi))):
                vis[f"{name}_extract_visible_ms"] = median_ms(lambda: m.extract_visible_points(pose, 100.0, hf, vf), warmup=3)
                steps = candidate_steps(e, voxel, pose, 100.0, hf, vf)
                vis[f"{name}_candidates"], vis[f"{name}_visible"] = len(steps), m.extract_visible_points(pose, 100.0, hf, vf).size()
                vis[f"{name}_mean_steps"] = round(float(steps.mean()), 1) if len(steps) else 0.0
                vis[f"{name}_max_steps"] = int(steps.max(initial=0))
print(json.dumps(out))
print(json.dumps(vis))
