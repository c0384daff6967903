"""Registration.align_batch against B sequential Registration.align_optimize calls, in one process on one GPU.

Shapes: (a) config 1 — a 1000-point random sample of the bundled source scan against the bundled target scan, both box-filtered
[0.5, 50] and voxel-downsampled at 0.25 m, k = 10 covariances, LM + Geman-McClure over the three annealing levels 10 / 5 / 2.5,
10 iterations a level; (b) the 900-point synthetic pair of the tests (gicp_pair at density 8), same optimiser.
The B initial guesses are seeded twists of up to 0.05 rad / 0.15 m around the identity (inside the basin of both pairs).

Both sides are timed with a host clock around calls that end in a stream synchronise (each align_optimize reads its result
back, align_batch reads all blocks back once); the source is prepared once, outside the timed region, for both. Per B: 3 warm-up
rounds, then `--reps` rounds that alternate batch and sequential; median, minimum and maximum in microseconds.
Usage: python profiles/time_align_batch.py [--reps 15] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,2,16,64,256,512")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_align_batch: needs a HIP device (a CPU run measures nothing)")
    import sycl_points_amd.api as sp
    from oracle.pyoracle import Oracle
    from sycl_points_amd.synthetic import gicp_pair
    from test_gpu_facade import GOLD, read_ply_xyz

    orc = Oracle()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    def covs(p, k):
        return orc.cov_estimate(p, orc.kdtree_knn(orc.kdtree_build(p), p, k)[0])

    def scan(name):
        p = read_ply_xyz(os.path.join(GOLD, name))
        p = p[orc.box_filter(p, 0.5, 50.0) == 1]
        p = orc.voxel_downsample(p, 0.25, 1, stable=True)["points"]
        return p, covs(p, 10)

    s, sc = scan("source.ply")
    t, tc = scan("target.ply")
    keep = orc.random_sampling_flags(1234, len(s), 1000) == 1
    pairs = {"config1-1000-of-bundled": (s[keep], sc[keep], t, tc)}
    r = 10.0 * (900 * 8.0 / 1e6) ** (1.0 / 3.0)
    src, tgt, _ = gicp_pair(900, r, 1234)
    pairs["synthetic-900"] = (src, covs(src, 20), tgt, covs(tgt, 20))

    scales = [10.0, 5.0, 2.5]
    params = sp.RegistrationParams(robust_type="GEMAN_MCCLURE", optimization_method="LM", max_iterations=10)
    rng = np.random.RandomState(7)
    batches = [int(b) for b in args.batches.split(",")]
    twists = rng.uniform(-1.0, 1.0, size=(max(batches), 6)) * np.array([0.05] * 3 + [0.15] * 3)
    guesses = [orc.se3_exp([float(v) for v in tw]) for tw in twists]
    rows = []
    for name, (ps, pcs, pt, pct) in pairs.items():
        S = sp.PointCloudShared(dev(ps), covs=dev(pcs))
        prep = sp.PreparedTarget(sp.GridKNN.build(dev(pt)), dev(pct))
        reg = sp.Registration(params)
        reg.align_optimize(S, prep, guesses[0], scales, True, prepare=True)  # prepares the source once for both sides
        for B in batches:
            G = guesses[:B]

            def batch():
                t0 = time.perf_counter()
                out = reg.align_batch(S, prep, G, scales, prepare=False)
                return (time.perf_counter() - t0) * 1e6, out

            def sequential():
                t0 = time.perf_counter()
                out = [reg.align_optimize(S, prep, T, scales, True, prepare=False) for T in G]
                return (time.perf_counter() - t0) * 1e6, out

            for _ in range(3):
                batch(), sequential()
            tb, ts = [], []
            for _ in range(args.reps):
                a, rb = batch()
                b, rs = sequential()
                tb.append(a)
                ts.append(b)
            assert all(x is not None for x in rs), "the single launch was not available"
            dpose = max(float(np.abs(x.T - y.T).max()) for x, y in zip(rb, rs))
            row = dict(pair=name, n=int(S.size()), target=int(len(pt)), B=B, batch_us=[float(np.median(tb)), float(min(tb)), float(max(tb))],
                       sequential_us=[float(np.median(ts)), float(min(ts)), float(max(ts))],
                       speedup=float(np.median(ts) / np.median(tb)), max_pose_difference=dpose,
                       steps_per_hypothesis=float(np.mean([x.linearizations + x.trials for x in rb])))
            rows.append(row)
            print(f"{name:26s} B={B:4d}  batch {row['batch_us'][0]:10.1f} us [{row['batch_us'][1]:.1f}, {row['batch_us'][2]:.1f}]   "
                  f"sequential {row['sequential_us'][0]:10.1f} us [{row['sequential_us'][1]:.1f}, {row['sequential_us'][2]:.1f}]   "
                  f"x{row['speedup']:.2f}   max |dT| {dpose:.1e}   steps/hyp {row['steps_per_hypothesis']:.1f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
