"""Voxelised GICP (Registration.align_voxel_map) against the path a submap pays for today, in one process on one GPU.

(a) the per-keyframe target cost. Existing: VoxelHashMap.downsampling (flag, scan, export kernels, one read-back) + KDTree.build on the
    export + a k = 10 search + covariance.estimate, which is what Submap::build_submap does before Registration::align can search its
    target. New: VoxelHashMap.prepare_registration (one launch over the table's slots). Maps: the bundled target scan (box filter
    [0.5, 50], voxel grid 0.25, k = 10 covariances) accumulated into 1 m voxels, and a synthetic map of about a million 1 m voxels.
(b) the per-iteration cost on the synthetic map: Registration.linearize_voxel_map with 1 / 7 / 27 probed cells at 1 k, 64 k and 1 M
    source points (voxel means moved by 0.1 m of noise and a small pose), against one iteration of the existing path on the same
    clouds: compute_linearized_result = a nearest-neighbour search of the map's export (KD-tree, and the GridKNN the facade puts in its
    place) + sp_gicp_linearize. Every call ends in the read-back of its 192-byte system, on both sides.

Host clock around calls that end in a stream synchronise; 3 warm-up rounds, then `--reps` rounds that alternate the contenders;
median, minimum and maximum in microseconds. Usage: python profiles/time_voxel_registration.py [--reps 21] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(us):
    return [float(np.median(us)), float(min(us)), float(max(us))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    ap.add_argument("--voxels", type=int, default=1000000)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_voxel_registration: needs a HIP device (a CPU run measures nothing)")
    import sycl_points_amd.api as sp
    from test_gpu_facade import GOLD, read_ply_xyz

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    sync = torch.cuda.synchronize

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return (time.perf_counter() - t0) * 1e6, out

    def alternate(contenders):
        for _ in range(3):
            for fn in contenders.values():
                timed(fn)
        us = {k: [] for k in contenders}
        for _ in range(args.reps):
            for k, fn in contenders.items():
                us[k].append(timed(fn)[0])
        return {k: stats(v) for k, v in us.items()}

    def with_covariances(points, k=10):
        c = sp.PointCloudShared(points)
        sp.covariance.estimate(sp.KDTree.build(c.points).knn_search(c.points, k), c)
        return c

    # ---- the two maps
    pts = dev(read_ply_xyz(os.path.join(GOLD, "target.ply")))
    pts = sp.compact_by_flags(pts, sp.box_filter_flags(pts, 0.5, 50.0)).contiguous()
    scan = with_covariances(sp.VoxelGrid(0.25).downsampling(sp.PointCloudShared(pts)).points.contiguous())
    bundled = sp.VoxelHashMap(1.0)
    bundled.add_point_cloud(scan)

    rs = np.random.RandomState(11)
    side = int(round(args.voxels ** (1.0 / 3.0)))
    cells = np.stack(np.meshgrid(*(np.arange(side),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    p = np.ones((len(cells), 4), np.float32)
    p[:, :3] = cells + rs.uniform(0.2, 0.8, cells.shape)
    p = p[rs.permutation(len(p))]
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    C = np.zeros((4, 4), np.float32)
    C[:3, :3] = q @ np.diag([0.01, 0.9, 1.1]) @ q.T
    big = sp.VoxelHashMap(1.0)
    big.set_rehash_threshold(0.3)
    done = 0
    while done < len(p):  # one rung of the capacity ladder per frame
        n = max(1, min(len(p) - done, int(0.3 * big.info("capacity"))))
        big.add_point_cloud(sp.PointCloudShared(dev(p[done:done + n]), covs=dev(np.broadcast_to(C.T.reshape(-1), (n, 16)))))
        done += n
    rows = []

    # ---- (a)
    for name, m in (("bundled target, 1 m voxels", bundled), (f"synthetic, {side}^3 voxels", big)):
        def existing():
            means = m.downsampling(distance=1e7)
            tree = sp.KDTree.build(means.points)
            sp.covariance.estimate(tree.knn_search(means.points, 10), means)
            return means

        res = alternate({"export + KDTree.build + k = 10 covariances": existing, "prepare_registration": lambda: m.prepare_registration("GICP")})
        row = dict(what="target per keyframe", map=name, voxels=m.info("voxel_num"), capacity=m.info("capacity"), us=res)
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- (b)
    means = big.downsampling(distance=1e7)
    tree, grid = sp.KDTree.build(means.points), sp.GridKNN.build(means.points)
    big.prepare_registration("GICP")
    host_means = means.points.cpu().numpy()
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.05, -0.03, 0.02]
    for n in (1000, 65536, 1000000):
        pick = rs.randint(0, len(host_means), n)
        s = host_means[pick].copy()
        s[:, :3] += rs.normal(0.0, 0.1, (n, 3)).astype(np.float32)
        S = sp.PointCloudShared(dev(s), covs=dev(np.broadcast_to(C.T.reshape(-1), (n, 16))))
        reg = sp.Registration(sp.RegistrationParams(max_correspondence_distance=1.0))
        reg.prepare_voxel_source(S)
        contenders = {f"voxel map, {c} cells": (lambda c=c: reg.linearize_voxel_map(S, big, T, neighbor_voxels=c, prepare_source=False))
                      for c in (1, 7, 27)}
        contenders["KD-tree search + linearise"] = lambda: reg.compute_linearized_result(S, means, tree, T)
        contenders["GridKNN search + linearise"] = lambda: reg.compute_linearized_result(S, means, grid, T)
        inliers = {k: (fn()["inlier"]) for k, fn in contenders.items()}
        res = alternate(contenders)
        row = dict(what="one linearisation", source_points=n, voxels=big.info("voxel_num"), us=res, inliers=inliers)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
