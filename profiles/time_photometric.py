"""The photometric term on one GPU, HIP-event medians.

  copy          a device-to-device copy of 512 MiB: the rate (bytes read + bytes written per second) the byte bounds are taken at
  gradient      sp_intensity_gradient at 1 M points (a curved sheet, grid order), k = 10 and 20, against
                  its byte bound    per point 4 k index + 20 k gathered (16 B point + 4 B intensity per neighbour) + 36 own + 16 written
                  K5                sp_cov_estimate on the same points and lists (4 k + 16 k + 64 written)
  linearize     sp_photometric_linearize at 64 k and 1 M correspondences (every source point has one), against
                  its byte bound    60 bytes per correspondence
                  sp_gicp_linearize POINT_TO_PLANE on the same correspondences (16 + 8 + 16 + 16 = 56 bytes per correspondence)
  error         sp_photometric_error on the same inputs
`--trace-only` runs 10 rounds of the device calls and measures nothing itself: the command to put under
`rocprofv3 --kernel-trace --stats` (the kernels' own times; no counters in the same run).
Events around `--inner` back-to-back calls, divided; 3 warm-up rounds, then `--reps` rounds; median, minimum and maximum in
microseconds.
Usage: python profiles/time_photometric.py [--reps 21] [--out profiles/photometric_timing.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_photometric: needs a HIP device (a CPU run measures nothing)")
    import f64_photometric as model
    import sycl_points_amd.api as sp
    from sycl_points_amd import _lib

    L = _lib.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    def measure(fn, inner=args.inner):
        us = []
        for rep in range(3 + args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(inner):
                fn()
            stop.record()
            stop.synchronize()
            if rep >= 3:
                us.append(start.elapsed_time(stop) * 1e3 / inner)
        return [float(np.median(us)), float(min(us)), float(max(us))]

    def sheet(n, seed):
        """a curved sheet of n points in grid order (neighbouring lanes gather neighbouring rows, as after a voxel filter)"""
        p, nr, it, _ = model.curved_sheet(n, seed, T=np.eye(4))
        c = sp.PointCloudShared(dev(p), normals=dev(nr), intensities=dev(it))
        return c.reordered(sp.GridKNN.build(c.points, points_per_cell=2.0).order().long())

    def gradient_case(n, k):
        c = sheet(n, 3)
        knn = sp.GridKNN.build(c.points, points_per_cell=2.0).self_knn(k)[0]
        idx = knn.indices if hasattr(knn, "indices") else knn
        return dict(c=c, idx=idx.contiguous(), k=k, n=n, rows=torch.empty((n, 4), dtype=torch.float32, device="cuda"),
                    covs=torch.empty((n, 16), dtype=torch.float32, device="cuda"))

    def gradient(d):
        sp.check(L.sp_intensity_gradient(ptr(d["c"].points), ptr(d["c"].normals), ptr(d["c"].intensities), d["n"], ptr(d["idx"]), d["k"],
                                         ptr(d["rows"]), stream()))

    def k5(d):
        sp.check(L.sp_cov_estimate(ptr(d["c"].points), d["n"], ptr(d["idx"]), d["k"], ptr(d["covs"]), stream()))

    def term_case(n):
        tgt = sheet(n, 5)
        src = sheet(n, 6)
        grid = sp.GridKNN.build(tgt.points, points_per_cell=2.0)
        rows = sp.intensity_gradients(grid.self_knn(10)[0], tgt)
        reg = sp.Registration(sp.RegistrationParams(reg_type="POINT_TO_PLANE", max_correspondence_distance=1.0))
        grid.nearest_neighbor_search_async(src, reg.neighbors, np.eye(4, dtype=np.float32))
        ws, lin = reg._buffers(src.points.device)
        return dict(src=src, tgt=tgt, rows=rows, reg=reg, ws=ws, lin=lin, n=n, grid=grid, T=np.eye(4, dtype=np.float32),
                    pp=sp.PhotometricParams(weight=1.0))

    def linearize(d):
        sp.photometric_linearize(d["src"], d["tgt"].points, d["rows"], d["reg"].neighbors, d["T"], d["pp"], 1.0, lin=d["lin"], workspace=d["ws"])

    def error(d):
        sp.photometric_error(d["src"], d["tgt"].points, d["rows"], d["reg"].neighbors, d["T"], d["pp"], 1.0, lin=d["lin"], workspace=d["ws"])

    def geometric(d):
        d["reg"]._linearize("linearize", d["src"], d["tgt"], d["T"], 10.0, d["lin"])

    if args.trace_only:
        for k in (10, 20):
            d = gradient_case(1 << 20, k)
            for _ in range(10):
                gradient(d), k5(d)
        for n in (1 << 16, 1 << 20):
            d = term_case(n)
            for _ in range(10):
                linearize(d), error(d), geometric(d)
        torch.cuda.synchronize()
        return
    out = {"reps": args.reps, "inner": args.inner}
    line = lambda tag, s, more="": print(f"{tag:44s} {s[0]:11.2f} us ({s[1]:.2f} .. {s[2]:.2f}) {more}", flush=True)  # noqa: E731

    a = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    s = measure(lambda: b.copy_(a), inner=4)
    rate = 2.0 * a.numel() / (s[0] * 1e-6)
    out["copy_512MiB"] = {"us": s, "bytes_per_second_read_plus_write": rate}
    line("copy 512 MiB", s, f"{rate / 1e12:.2f} TB/s read + write")
    del a, b

    for k in (10, 20):
        d = gradient_case(1 << 20, k)
        n = d["n"]
        sg, sk = measure(lambda: gradient(d)), measure(lambda: k5(d))
        bound = n * (4.0 * k + 20.0 * k + 36.0 + 16.0) / rate * 1e6
        bound_k5 = n * (4.0 * k + 16.0 * k + 64.0) / rate * 1e6
        out[f"gradient_1M_k{k}"] = {"us": sg, "byte_bound_us": bound, "fraction_of_bound": bound / sg[0], "k5_us": sk,
                                    "k5_byte_bound_us": bound_k5, "k5_fraction_of_bound": bound_k5 / sk[0]}
        line(f"gradient, 1 M points, k = {k}", sg, f"byte bound {bound:.1f} us ({100 * bound / sg[0]:.1f} %)")
        line(f"K5 (sp_cov_estimate), same lists", sk, f"byte bound {bound_k5:.1f} us ({100 * bound_k5 / sk[0]:.1f} %)")
        del d
    for n in (1 << 16, 1 << 20):
        d = term_case(n)
        sl, se, sgeo = measure(lambda: linearize(d)), measure(lambda: error(d)), measure(lambda: geometric(d))
        bound, bound_geo = n * 60.0 / rate * 1e6, n * 56.0 / rate * 1e6
        out[f"term_{n}"] = {"linearize_us": sl, "error_us": se, "byte_bound_us": bound, "linearize_fraction_of_bound": bound / sl[0],
                            "error_fraction_of_bound": bound / se[0], "gicp_linearize_point_to_plane_us": sgeo,
                            "gicp_linearize_byte_bound_us": bound_geo}
        line(f"photometric linearize, {n} correspondences", sl, f"byte bound {bound:.2f} us ({100 * bound / sl[0]:.1f} %)")
        line(f"photometric error, {n} correspondences", se, f"byte bound {bound:.2f} us ({100 * bound / se[0]:.1f} %)")
        line(f"sp_gicp_linearize POINT_TO_PLANE, same", sgeo, f"byte bound {bound_geo:.2f} us ({100 * bound_geo / sgeo[0]:.1f} %)")
        del d
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
