"""Registration.align_voxel_map_batch (one launch, a workgroup per guess) against B sequential Registration.align_voxel_map calls
(the host-driven loop: two launches and a read-back per linearisation and per trial), in one process on one GPU.

Scenes: (a) the three planes of tests/test_gpu_voxel_registration.py, 1000 source points, 0.5 m voxels; (b) the bundled pair (box
filter [0.5, 50], voxel grid 0.25, k = 10 covariances), the target accumulated into 1 m voxels. LM + GICP + Geman-McClure, 1 cell.
Guesses: small twists around the identity, inside the basin, so that every hypothesis does an alignment's worth of work.
B in {1, 2, 4, 16, 64, 256}. Host clock around calls that end in a stream synchronise; 3 warm-up rounds, then `--reps` rounds
that alternate the two contenders; median, minimum and maximum in microseconds.
Usage: python profiles/time_voxel_align_batch.py [--reps 21] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BATCHES = (1, 2, 4, 16, 64, 256)


def stats(us):
    return [float(np.median(us)), float(min(us)), float(max(us))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_voxel_align_batch: needs a HIP device (a CPU run measures nothing)")
    from scipy.linalg import expm

    import f64_factors as f64
    import sycl_points_amd.api as sp
    from test_gpu_facade import GOLD, read_ply_xyz
    from test_gpu_voxel_registration import planes_scene, with_covariances

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    sync = torch.cuda.synchronize

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return (time.perf_counter() - t0) * 1e6, out

    def guesses(B, seed=7):
        rs = np.random.RandomState(seed)
        return [expm(f64.twist_matrix(rs.uniform(-1.0, 1.0, 6) * np.array([0.01, 0.01, 0.01, 0.05, 0.05, 0.05]))).astype(np.float32)
                for _ in range(B)]

    def scene_planes():
        tgt, src, _ = planes_scene()
        m = sp.VoxelHashMap(0.5)
        m.add_point_cloud(with_covariances(sp, tgt))
        return with_covariances(sp, src[:1000]), m, dict(max_correspondence_distance=1.0, robust_default_scale=1.0)

    def scene_bundled():
        def prep(name):
            pts = dev(read_ply_xyz(os.path.join(GOLD, name)))
            pts = sp.compact_by_flags(pts, sp.box_filter_flags(pts, 0.5, 50.0)).contiguous()
            c = sp.VoxelGrid(0.25).downsampling(sp.PointCloudShared(pts))
            return with_covariances(sp, c.points.contiguous().cpu().numpy())

        m = sp.VoxelHashMap(1.0)
        m.add_point_cloud(prep("target.ply"))
        return prep("source.ply"), m, dict(max_correspondence_distance=2.0, robust_default_scale=2.5)

    out = {"reps": args.reps, "scenes": {}}
    for name, make in (("planes_1000", scene_planes), ("bundled_pair", scene_bundled)):
        source, m, kw = make()
        params = lambda: sp.RegistrationParams(reg_type="GICP", optimization_method="LM", robust_type="GEMAN_MCCLURE",  # noqa: E731
                                               max_iterations=30, **kw)
        batch_reg, seq_reg = sp.Registration(params()), sp.Registration(params())
        rows = {}
        for B in BATCHES:
            G = guesses(B)
            contenders = {"batch": lambda: batch_reg.align_voxel_map_batch(source, m, G),
                          "sequential": lambda: [seq_reg.align_voxel_map(source, m, T) for T in G]}
            for _ in range(3):
                for fn in contenders.values():
                    timed(fn)
            us = {k: [] for k in contenders}
            res = {}
            for _ in range(args.reps):
                for k, fn in contenders.items():
                    t, res[k] = timed(fn)
                    us[k].append(t)
            steps = [r.linearizations + r.trials for r in res["batch"]]
            dT = max(float(np.abs(a.T - b.T).max()) for a, b in zip(res["batch"], res["sequential"]))
            rows[B] = {"batch_us": stats(us["batch"]), "sequential_us": stats(us["sequential"]), "steps_per_guess": float(np.mean(steps)),
                       "max_pose_difference": dT}
            print(f"{name:13s} n={source.size():5d} B={B:3d}  batch {rows[B]['batch_us'][0]:9.1f} us ({rows[B]['batch_us'][1]:.1f} .. "
                  f"{rows[B]['batch_us'][2]:.1f})  sequential {rows[B]['sequential_us'][0]:10.1f} us ({rows[B]['sequential_us'][1]:.1f} .. "
                  f"{rows[B]['sequential_us'][2]:.1f})  ratio {rows[B]['sequential_us'][0] / rows[B]['batch_us'][0]:6.2f}  "
                  f"steps/guess {rows[B]['steps_per_guess']:.1f}  max |dT| {dT:.1e}", flush=True)
        out["scenes"][name] = {"source_points": source.size(), "voxels": m.info("voxel_num"), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
