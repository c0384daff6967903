"""The stages of the global registration in one process on one GPU.

  fpfh        sp_fpfh_compute, k = 20: the bundled target at 0.5 m voxels (about 2 700 points) and 65 536 points of a synthetic scene
              (points scattered on two walls, a floor and a ceiling, normals towards the origin)
  match       sp_feature_match on the same descriptors, n x n; at 65 536 x 65 536 also the share of the f32 matrix-core peak
              (157.3 TFLOP/s) the whole call reaches, counting the 2 x 34 flops per pair the 17 MFMA steps execute
  score       sp_ransac_score, 50 000 hypotheses over 465 matches
  align_global  end to end on the bundled pair at 1 m voxels, the source turned by 150 degrees (match, score, select, 64 guesses
              through align_batch, best_of), against align_batch from a yaw sweep of 36 guesses on the same clouds
Host clock around calls that end in a stream synchronise; 3 warm-up rounds, then `--reps` rounds; median, minimum and maximum in
microseconds.
Usage: python profiles/time_global_registration.py [--reps 21] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_F32_MFMA = 157.3e12


def stats(us):
    return [float(np.median(us)), float(min(us)), float(max(us))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_global_registration: needs a HIP device (a CPU run measures nothing)")
    import f64_fpfh as model
    import sycl_points_amd.api as sp

    gold = os.path.join(ROOT, "tests", "golden")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    sync = torch.cuda.synchronize

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return (time.perf_counter() - t0) * 1e6, out

    def measure(fn):
        for _ in range(3):
            timed(fn)
        us, out = [], None
        for _ in range(args.reps):
            t, out = timed(fn)
            us.append(t)
        return stats(us), out

    def with_lists(xyz, k=20):
        """cloud with covariances, normals towards the sensor and its own k-NN lists"""
        p = np.ones((len(xyz), 4), np.float32)
        p[:, :3] = xyz
        c = sp.PointCloudShared(dev(p))
        tree = sp.KDTree.build(c.points)
        knn = tree.knn_search(c, k)
        sp.covariance.estimate(knn, c)
        nrm = sp.covariance.estimate_normals(tree.knn_search(c, 10), c)
        away = (nrm[:, :3] * c.points[:, :3]).sum(1, keepdim=True) > 0
        c.normals = torch.where(away, -nrm, nrm).contiguous()
        return c, knn, tree

    def scan(name, voxel, turn=None):
        pts = dev(model.read_ply_xyz(os.path.join(gold, name)))
        pts = sp.compact_by_flags(pts, sp.box_filter_flags(pts, 0.5, 50.0)).contiguous()
        xyz = sp.VoxelGrid(voxel).downsampling(sp.PointCloudShared(pts)).points.contiguous().cpu().numpy()[:, :3]
        if turn is not None:
            xyz = (xyz.astype(np.float64) @ turn[:3, :3].T).astype(np.float32)
        return with_lists(xyz)

    def synthetic(n, seed=3):
        """two walls, a floor and a ceiling around the sensor, 2 cm of noise"""
        rs = np.random.RandomState(seed)
        u, v, far = rs.uniform(-20, 20, n), rs.uniform(-20, 20, n), np.full(n, 20.0)
        surfaces = [(far, u, 0.2 * v), (u, far, 0.2 * v), (u, v, np.full(n, -2.0)), (u, v, np.full(n, 6.0))]
        pick = rs.randint(0, 4, n)
        xyz = np.stack([np.choose(pick, [sf[a] for sf in surfaces]) for a in range(3)], 1)
        return with_lists(xyz + rs.normal(0, 0.02, xyz.shape))

    out = {"reps": args.reps}
    line = lambda tag, s: print(f"{tag:44s} {s[0]:11.1f} us ({s[1]:.1f} .. {s[2]:.1f})", flush=True)  # noqa: E731

    small, small_knn, _ = scan("target.ply", 0.5)
    big, big_knn, _ = synthetic(65536)
    feats = {}
    for tag, (c, knn) in (("small", (small, small_knn)), ("big", (big, big_knn))):
        s, feats[tag] = measure(lambda: sp.fpfh(knn, c))
        out[f"fpfh_{c.size()}"] = s
        line(f"fpfh n = {c.size()}, k = 20", s)
    for tag, c in (("small", small), ("big", big)):
        f = feats[tag]
        s, _ = measure(lambda: sp.match_features(f, f))
        n = c.size()
        flops = float(n) * n * 2 * 34
        out[f"match_{n}x{n}"] = {"us": s, "tflops_executed": flops / (s[0] * 1e-6) / 1e12, "share_of_f32_mfma_peak": flops / (s[0] * 1e-6) / PEAK_F32_MFMA}
        line(f"match {n} x {n}", s)
        print(f"{'':44s} {flops / (s[0] * 1e-6) / 1e12:9.2f} TFLOP/s executed, {100 * flops / (s[0] * 1e-6) / PEAK_F32_MFMA:.1f} % of the f32 MFMA peak")

    rs = np.random.RandomState(1)
    cs = np.ones((465, 4), np.float32)
    cs[:, :3] = rs.uniform(-30, 30, (465, 3))
    ct = cs.copy()
    ct[:, :3] += rs.normal(0, 0.2, (465, 3))
    cs_d, ct_d = dev(cs), dev(ct)
    s, _ = measure(lambda: sp.ransac_scores(cs_d, ct_d, 50000, 1.0, 0.0, 0.9, 1))
    out["score_50000_x_465"] = s
    line("score 50 000 hypotheses x 465 matches", s)

    Rz = model.rot_z(150.0)
    T_true = np.loadtxt(os.path.join(gold, "T_target_source.txt")) @ np.linalg.inv(Rz)
    src, src_knn, _ = scan("source.ply", 1.0, Rz)
    tgt, tgt_knn, _ = scan("target.ply", 1.0)
    fs, ft = sp.fpfh(src_knn, src), sp.fpfh(tgt_knn, tgt)
    prep = sp.PreparedTarget(sp.GridKNN.build(tgt.points), tgt.covs)
    params = lambda: sp.RegistrationParams(reg_type="GICP", max_correspondence_distance=2.0, max_iterations=30)  # noqa: E731
    gp = sp.GlobalRegistrationParams(hypotheses=50000, guesses=64, inlier_distance=1.0, seed=2024)
    reg_g, reg_s = sp.Registration(params()), sp.Registration(params())
    sweep = [model.rot_z(10.0 * k).astype(np.float32) for k in range(36)]
    s, res = measure(lambda: reg_g.align_global(src, fs, tgt, ft, prep, gp))
    s2, swept = measure(lambda: reg_s.align_batch(src, prep, sweep))
    s3, _ = measure(lambda: (sp.fpfh(src_knn, src), sp.fpfh(tgt_knn, tgt)))
    best = sp.Registration.best_of(swept)
    eg = model.pose_errors(res.T, T_true)
    es = model.pose_errors(swept[best].T, T_true) if best < len(swept) else (float("nan"), float("nan"))
    out["bundled_pair_1m"] = {"source_points": src.size(), "target_points": tgt.size(), "align_global_us": s, "yaw_sweep_36_us": s2,
                              "fpfh_both_clouds_us": s3, "align_global_error_m_rad": eg, "yaw_sweep_error_m_rad": es}
    line(f"align_global, {src.size()} / {tgt.size()} points", s)
    line("align_batch, yaw sweep of 36 guesses", s2)
    line("fpfh of both clouds (not in align_global)", s3)
    print(f"errors against the truth: align_global {eg[0]:.3f} m {eg[1]:.4f} rad | yaw sweep {es[0]:.3f} m {es[1]:.4f} rad")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
