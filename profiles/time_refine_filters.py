"""The scan filters that follow kNN and covariances: every instantiation of the three kernels on 1 000 000 points of noisy planes
(neighbours from the library's KDTree, k = 10 and 20; covariances and normals from the library), 20 calls each after 3 of warm-up,
and K5 (sp_cov_estimate) at the same k beside the gather kernel. Meant to run under `rocprofv3 --kernel-trace --stats -- python
profiles/time_refine_filters.py`, whose per-kernel statistics are the figures DESIGN.md quotes; by itself it writes the HIP-event
medians to profiles/refine_filters_timing.json (or the path given as its argument) and prints them as one JSON line. Rates are
algorithmic bytes per point over time, to set against the 6.29 TB/s copy rate of SURVEY.md section 8d. Run from the repository root."""
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


def planes(n, seed=7):
    rs = np.random.RandomState(seed)
    side = np.sqrt(n / 3.0) * 0.1
    uv = rs.uniform(-0.5 * side, 0.5 * side, (n, 2)).astype(np.float32)
    noise = rs.normal(0.0, 0.01, n).astype(np.float32)
    pts = np.ones((n, 4), np.float32)
    which = np.arange(n) % 3
    for w, (axis, offset) in enumerate(((2, -1.5), (0, 3.0), (1, -2.5))):
        m = which == w
        others = [a for a in range(3) if a != axis]
        pts[m, others[0]], pts[m, others[1]], pts[m, axis] = uv[m, 0], uv[m, 1], offset + noise[m]
    return pts[rs.permutation(n)]  # (no spatial order: the gather's worst case)


def timed(call):
    for _ in range(3):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    for a, b in ev:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3


def main():
    L = _lib.lib()
    torch.cuda.set_device(0)
    n = 1_000_000
    pts = torch.from_numpy(planes(n)).cuda()
    inten = torch.rand(n, device="cuda") * 255
    out_i = torch.empty_like(inten)
    flags = torch.empty(n, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
    tree = sp.KDTree.build(pts)
    knn = {k: tree.knn_search(pts, k).indices for k in (10, 20)}
    covs = sp.covariance.estimate(knn[10], pts)
    nrm = sp.covariance.extract_normals(pts, covs)
    out = {"n": n, "device": torch.cuda.get_device_name(0), "timing": "median of 20 calls after 3 warm-up (HIP events)"}

    def row(name, bytes_per_point, call):
        def checked():
            assert call() == 0
        us = timed(checked)
        out[name] = {"bytes_per_point": bytes_per_point, "event_us": round(us, 2), "TB_per_s": round(bytes_per_point * n / us * 1e-6, 3)}

    row("angle_flags normals", 33, lambda: L.sp_angle_incidence_flags(p(pts), p(nrm), None, n, 0.2, 1.2, p(flags), st))
    row("angle_flags covs", 65, lambda: L.sp_angle_incidence_flags(p(pts), None, p(covs), n, 0.2, 1.2, p(flags), st))
    for name, b, nr, cv, ae in (("correct distance", 24, None, None, 0.0), ("correct normals", 40, nrm, None, 1.0), ("correct covs", 72, None, covs, 1.0)):
        row(name, b, lambda nr=nr, cv=cv, ae=ae: L.sp_intensity_correct(p(pts), p(nr), p(cv), p(inten), n, 0.0, 1.0, 0.0, 1000.0, 1.0, ae, st))
    cov_out = torch.empty((n, 16), device="cuda")
    for k in (10, 20):
        bpp = 24 * k + 24
        for name, mean_min in (("smooth", 0.0), ("local mean", 1e-3)):
            row(f"gaussian {name} k={k} (16-byte rows)" if k % 4 == 0 else f"gaussian {name} k={k} (dword rows)", bpp,
                lambda k=k, mean_min=mean_min: L.sp_intensity_gaussian(p(pts), p(inten), p(knn[k]), n, k, k, 0.1, 0.1, 0.05, mean_min, p(out_i), st))
        row(f"K5 sp_cov_estimate k={k}", 20 * k + 64, lambda k=k: L.sp_cov_estimate(p(pts), n, p(knn[k]), k, p(cov_out), st))
    row("gaussian smooth k=10 of stride 20 (16-byte rows)", 264, lambda: L.sp_intensity_gaussian(p(pts), p(inten), p(knn[20]), n, 20, 10, 0.1, 0.1, 0.05, 0.0, p(out_i), st))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "refine_filters_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
