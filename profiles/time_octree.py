"""The device-built octree on the 1 M-point non-uniform cloud of tests/test_gpu_bvh.py (planes + a dense cluster), one JSON line per
step. Steps (one process each, so that profiles/time_octree.sh can give each its own time limit):
  build   sp_octree_create at 1 M points (resolution 0.1, 32 points per node): median of 10 wall times, each with its synchronise
          (the create synchronises), beside sp_bvh_create
  k20     k = 20, the cloud's own 1 M points as external queries: Octree beside BVH (median of 5, HIP events)
  k40     k = 40, every tenth point (100 k queries): Octree (build + search, and the search alone) beside the accelerated KDTree,
          whose k > 32 is answered by the host-built tree: its first search includes that host build, the second does not
  k100    the same at k = 100
Run from the repository root: bash profiles/time_octree.sh"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sycl_points_amd.api as sp  # noqa: E402


def nonuniform_cloud(n, seed=7):  # tests/test_gpu_bvh.py
    rs = np.random.RandomState(seed)
    m = n // 5
    parts = []
    for axis in range(3):
        p = rs.uniform(-40, 40, (m, 3))
        p[:, axis] = rs.normal(0.0, 0.01, m)
        parts.append(p)
    parts.append(rs.uniform(-40, 40, (n - 4 * m, 3)) * np.array([1.0, 1.0, 0.1]))
    c = rs.normal(0.0, 1.0, (m, 3))
    parts.append(np.array([3.0, -2.0, 1.0]) + 0.2 * c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-9) * rs.uniform(0, 1, (m, 1)) ** (1 / 3))
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = np.concatenate(parts)[:n].astype(np.float32)
    return pts


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_ms(fn, runs=5, warmup=1):
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


def main():
    step = sys.argv[1]
    torch.cuda.set_device(0)
    n = 1_000_000
    pts = torch.from_numpy(nonuniform_cloud(n)).cuda()
    out = {"step": step, "n": n}
    if step == "build":
        sp.Octree.build(pts, 0.1, 32)
        sp.BVH.build(pts)
        out["octree_build_ms"] = float(np.median([wall_ms(lambda: sp.Octree.build(pts, 0.1, 32))[0] for _ in range(10)]))
        out["bvh_build_ms"] = float(np.median([wall_ms(lambda: sp.BVH.build(pts))[0] for _ in range(10)]))
        t = sp.Octree.build(pts, 0.1, 32)
        out.update(nodes=t.info("nodes"), leaves=t.info("leaves"), depth=t.info("depth"))
    elif step == "k20":
        oct_, bvh = sp.Octree.build(pts, 0.1, 32), sp.BVH.build(pts)
        ro, rb = sp.KNNResult(), sp.KNNResult()
        out["nq"] = n
        out["octree_search_ms"] = event_ms(lambda: oct_.knn_search_async(pts, 20, ro))
        out["bvh_search_ms"] = event_ms(lambda: bvh.knn_search_async(pts, 20, rb))
        out["same_rows"] = bool(torch.equal(ro.indices, rb.indices) and torch.equal(ro.distances, rb.distances))
    else:
        k = {"k40": 40, "k100": 100}[step]
        q = pts[::10].contiguous()
        out.update(k=k, nq=int(q.shape[0]))
        ro, rk = sp.KNNResult(), sp.KNNResult()
        out["octree_build_ms"], oct_ = wall_ms(lambda: sp.Octree.build(pts, 0.1, 32))
        out["octree_search_ms"] = event_ms(lambda: oct_.knn_search_async(q, k, ro))
        tree = sp.KDTree.build(pts, accelerate=True)
        out["kdtree_first_search_with_host_build_ms"] = wall_ms(lambda: tree.knn_search_async(q, k, rk))[0]
        out["kdtree_search_ms"] = event_ms(lambda: tree.knn_search_async(q, k, rk), runs=3, warmup=0)
        out["same_distances"] = bool(torch.equal(ro.distances, rk.distances))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
