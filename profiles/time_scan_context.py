"""Scan Context place recognition on one GPU, HIP-event medians.

  copy        a device-to-device copy of 512 MiB: the rate (bytes read + bytes written per second) the bounds below are taken at
  compute     sp_scan_context_compute on 131 072 points, against 16 bytes a point at the copy rate
  add         sp_scan_context_db_add of one descriptor
  search      sp_scan_context_db_search at N = 10^3, 10^4, 10^5 entries, k = 10 (normalise, search, select: the whole call), against
              the entry's bytes at the copy rate and 2 x 64 x 64 x K_pad FLOP an entry at the f32 matrix-core peak (157.3 TFLOP/s)
  search, vector unit   the same searches with the products on the vector unit (csrc/sp_internal.h:
              sp_internal_scan_context_search_form(1)): the A/B measurement of DESIGN.md 4.21
`--trace-only` runs 20 computes and 20 searches of each form at N = 10^5 and measures nothing itself: the command to put under
`rocprofv3 --kernel-trace --stats` (the kernels' own times) or `rocprofv3 --pmc` (counters, a run of their own).
Events around `--inner` back-to-back calls, divided; 3 warm-up rounds, then `--reps` rounds; median, minimum and maximum in
microseconds.
Usage: python profiles/time_scan_context.py [--reps 21] [--out profiles/scan_context_timing.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_F32_MFMA = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_scan_context: needs a HIP device (a CPU run measures nothing)")
    import f64_scan_context as model
    import sycl_points_amd.api as sp

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

    from sycl_points_amd import _lib

    set_form = _lib.lib().sp_internal_scan_context_search_form
    if args.trace_only:
        p = sp.ScanContextParams()
        pts = torch.from_numpy(model.scan(131072, 1)).cuda()
        D = sp.scan_context(pts, p)
        db = sp.ScanContextDatabase(p, capacity_hint=100000)
        for i in range(100000):
            db.add(D)
        for form in (0, 1):
            set_form(form)
            for _ in range(20):
                sp.scan_context(pts, p)
                db.search(D, 10)
        set_form(0)
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

    p = sp.ScanContextParams()
    pts = torch.from_numpy(model.scan(131072, 1)).cuda()
    s = measure(lambda: sp.scan_context(pts, p))
    bound = 16.0 * pts.shape[0] / rate * 1e6
    out["compute_131072"] = {"us": s, "bound_us": bound, "fraction_of_bound": bound / s[0]}
    line("compute, 131 072 points", s, f"bound {bound:.2f} us: {100 * bound / s[0]:.1f} %")

    D = sp.scan_context(pts, p)
    scratch_db = sp.ScanContextDatabase(p, capacity_hint=1 << 12)

    def add_one():
        if scratch_db.size() >= (1 << 12):
            scratch_db.clear()
        scratch_db.add(D)

    s = measure(add_one)
    out["add"] = {"us": s}
    line("add", s)

    rs = np.random.RandomState(2)
    pool = [torch.from_numpy((rs.uniform(0.05, 12.0, (20, 60)) * (rs.uniform(size=(20, 60)) < 0.3)).astype(np.float32)).cuda()
            for _ in range(64)]
    k_pad, tiles = (p.rings + 3) // 4 * 4, 2 if p.sectors > 32 else 1
    entry_bytes = k_pad * 32 * tiles * 4 + 8
    flop = 2.0 * (32 * tiles) ** 2 * k_pad
    for n in (1000, 10000, 100000):
        db = sp.ScanContextDatabase(p, capacity_hint=n)
        for i in range(n):
            db.add(pool[i % 64])
        s = measure(lambda: db.search(D, 10))
        mem, mfma = n * entry_bytes / rate * 1e6, n * flop / PEAK_F32_MFMA * 1e6
        out[f"search_{n}"] = {"us": s, "bytes_per_entry": entry_bytes, "flop_per_entry": flop, "memory_bound_us": mem,
                              "mfma_bound_us": mfma, "fraction_of_memory_bound": mem / s[0], "fraction_of_mfma_bound": mfma / s[0]}
        line(f"search N = {n}, k = 10", s, f"memory bound {mem:.2f} us ({100 * mem / s[0]:.1f} %), MFMA bound {mfma:.2f} us "
                                            f"({100 * mfma / s[0]:.1f} %)")
        set_form(1)
        v = measure(lambda: db.search(D, 10))
        set_form(0)
        out[f"search_{n}"]["vector_unit_form_us"] = v
        line(f"search N = {n}, k = 10, vector unit", v)
        del db
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
