"""OccupancyGridMap on the bundled scan (tests/golden/target.ply, 69 088 points, sensor at the origin) at voxel 0.25 m and 1.0 m:
add_point_cloud with carving off and on, and extract_occupied_points. HIP-event medians of 20 calls after 5 of warm-up, for the
first frame into a cleared map (the clear outside the events; with carving this includes the growth rehash) and for the same scan
added again to the grown map (the steady state of a submap). Also the voxel count, capacity and misses per ray. One JSON line."""
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
print(json.dumps(out))
