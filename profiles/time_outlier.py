"""The outlier filters and the intensity z-score at 1 M points, k = 10 and 20, in one process: one JSON line.

Cloud: 1 048 576 points of the three noisy planes of tests/test_refine_filters_cpu.py's planes_cloud (about 0.1 apart), intensities
U[0, 255). Per k: the median of 30 calls (after 5 of warm-up, timed by HIP events) of sp_outlier_statistical_flags (its three
launches), sp_outlier_radius_flags and sp_intensity_zscore on a kNN result that is already on the device, beside them the byte bound
of DESIGN.md section 4.11 at the measured copy rate of the part (6.29 TB/s), and the time of the sp_knn_tree_search call that produces
the input at the same n and k. Run from the repository root: python profiles/time_outlier.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sycl_points_amd.api as sp  # noqa: E402
from sycl_points_amd import _lib  # noqa: E402

COPY_RATE = 6.29e12  # bytes per second, the measured copy rate of an MI355X


def planes(n, seed=2024):
    rs = np.random.RandomState(seed)
    side = np.sqrt(n / 3.0) * 0.1
    uv = rs.uniform(-0.5 * side, 0.5 * side, (n, 2))
    noise = rs.normal(0.0, 0.01, n)
    which = np.arange(n) % 3
    pts = np.ones((n, 4), np.float32)
    for w, (axis, offset) in enumerate(((2, -1.5), (0, 3.0), (1, -2.5))):
        m = which == w
        others = [a for a in range(3) if a != axis]
        pts[m, others[0]] = uv[m, 0]
        pts[m, others[1]] = uv[m, 1]
        pts[m, axis] = offset + noise[m]
    return pts, rs.uniform(0.0, 255.0, n).astype(np.float32)


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


def bound_ms(bytes_per_point, n):
    return bytes_per_point * n / COPY_RATE * 1e3


def main():
    L = _lib.lib()
    torch.cuda.set_device(0)
    n = 1 << 20
    pts, inten = planes(n)
    P, I = torch.from_numpy(pts).cuda(), torch.from_numpy(inten).cuda()
    tree = sp.KDTree.build(P, accelerate=True)
    out = {"points": n, "copy_rate_TB_s": COPY_RATE / 1e12,
           "timing": "median of 30 C-ABI calls after 5 warm-up (HIP events); bound: the bytes of DESIGN.md 4.11 at the copy rate"}
    flags = torch.empty(n, dtype=torch.uint8, device="cuda")
    mean = torch.empty(n, dtype=torch.float32, device="cuda")
    stats = torch.empty(4, dtype=torch.float32, device="cuda")
    zout = torch.empty(n, dtype=torch.float32, device="cuda")
    nbytes = L.sp_outlier_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for k in (10, 20):
        res = sp.KNNResult()
        tree.knn_search_async(P, k, res)
        torch.cuda.synchronize()
        d2, idx = res.distances, res.indices
        radius = float(d2[:, k - 1].median())

        def search():
            tree.knn_search_async(P, k, res)

        def statistical():
            _lib.check(L.sp_outlier_statistical_flags(sp._ptr(d2), n, k, k, 1.0, sp._ptr(flags), sp._ptr(mean), sp._ptr(stats), sp._ptr(ws),
                                                      nbytes, sp._stream()))

        def radius_flags():
            _lib.check(L.sp_outlier_radius_flags(sp._ptr(d2), n, k, k - 1, radius, sp._ptr(flags), sp._stream()))

        def zscore():
            _lib.check(L.sp_intensity_zscore(sp._ptr(I), sp._ptr(idx), n, k, k, 0.01, sp._ptr(zout), sp._stream()))

        row = {"knn_backend": tree.backend_for(P, k), "knn_tree_search_ms": median_ms(search),
               "statistical": {"ms": median_ms(statistical), "launches": 3, "bytes_per_point": 4 * k + 13, "bound_ms": bound_ms(4 * k + 13, n)},
               "radius": {"ms": median_ms(radius_flags), "launches": 1, "bytes_per_point": 4 * k + 1, "bound_ms": bound_ms(4 * k + 1, n)},
               "zscore": {"ms": median_ms(zscore), "launches": 1, "bytes_per_point": 8 * k + 8, "bound_ms": bound_ms(8 * k + 8, n)}}
        statistical()
        torch.cuda.synchronize()
        row["statistical"]["removed"] = int(n - int(flags.sum()))
        row["statistical"]["stats"] = [float(v) for v in stats.cpu()]
        row["chain_over_search"] = row["statistical"]["ms"] / row["knn_tree_search_ms"]
        out[f"k{k}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
