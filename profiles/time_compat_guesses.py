"""Compatibility-graph guesses on one GPU, HIP-event medians, at M = 256, 1024, 4096 and 8192 matches (2 % of
them inliers, tests/f64_compat.py: hall_matches).

  copy          a device-to-device copy of 512 MiB: the rate (bytes read + bytes written per second) the memory bound is taken at
  seeds         sp_compat_seeds (zero, compat_kernel, second_order_kernel, seed_rank_kernel: the whole call), 64 seeds, against
                  memory bound   C written once and read once, 2 Mp^2 bytes (Mp = M rounded up to 128), at the copy rate
                  MFMA bound     M^3 multiply-adds at the int8 matrix-core peak, 2 x the dense BF16 peak of 2.5 PFLOP/s = 2.5e15 MAC/s
  consensus     sp_compat_consensus, 64 seeds of 16 companions (seed_rows_kernel, consensus_kernel)
  pose_score    sp_pose_score of 64 poses
  host          sp_compat_poses_host + sp_compat_select_host on host copies (wall clock, median)
  guesses       api.compat_guesses: everything above with its two read-backs and the upload of the poses (wall clock, median)
  ransac_score  sp_ransac_score of 50 000 triplets on the same matches: the yardstick (that kernel is not touched by 4.22)
`--trace-only` runs 10 rounds of the four device calls at every M and measures nothing itself: the command to put under
`rocprofv3 --kernel-trace --stats` (the kernels' own times; no counters in the same run).
Events around `--inner` back-to-back calls, divided; 3 warm-up rounds, then `--reps` rounds; median, minimum and maximum in
microseconds.
Usage: python profiles/time_compat_guesses.py [--reps 21] [--out profiles/compat_guesses_timing.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_I8_MAC = 2.5e15
SIZES = (256, 1024, 4096, 8192)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_compat_guesses: needs a HIP device (a CPU run measures nothing)")
    import f64_compat as model
    import sycl_points_amd.api as sp
    from sycl_points_amd import _lib

    L = _lib.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

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

    def wall(fn, reps=7):
        us = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) * 1e6)
        return [float(np.median(us)), float(min(us)), float(max(us))]

    def case(m):
        cs, ct, _, _ = model.hall_matches(m, max(m // 50, 5), 3)
        d = dict(m=m, cs_host=cs, ct_host=ct, cs=torch.from_numpy(cs).cuda(), ct=torch.from_numpy(ct).cuda())
        d["ws"] = torch.empty(L.sp_compat_workspace_bytes(m), dtype=torch.uint8, device="cuda")
        d["seed_idx"] = torch.empty(64, dtype=torch.int32, device="cuda")
        d["seed_s"] = torch.empty(64, dtype=torch.int32, device="cuda")
        d["cons"] = torch.empty((64, 16), dtype=torch.int32, device="cuda")
        d["poses"] = torch.eye(4, dtype=torch.float32, device="cuda").repeat(64, 1, 1).reshape(64, 16).contiguous()
        d["score"] = torch.empty(64, dtype=torch.int32, device="cuda")
        d["rscore"] = torch.empty(50000, dtype=torch.int32, device="cuda")
        return d

    def seeds(d):
        sp.check(L.sp_compat_seeds(ptr(d["cs"]), ptr(d["ct"]), d["m"], 0.1, 1.0, 64, ptr(d["seed_idx"]), ptr(d["seed_s"]), None, None,
                                   ptr(d["ws"]), d["ws"].numel(), stream()))

    def consensus(d):
        sp.check(L.sp_compat_consensus(d["m"], ptr(d["seed_idx"]), 64, 16, ptr(d["cons"]), None, ptr(d["ws"]), d["ws"].numel(), stream()))

    def pose_score(d):
        sp.check(L.sp_pose_score(ptr(d["cs"]), ptr(d["ct"]), d["m"], ptr(d["poses"]), 64, 0.3, ptr(d["score"]), stream()))

    def ransac(d):
        sp.check(L.sp_ransac_score(ptr(d["cs"]), ptr(d["ct"]), d["m"], 50000, 2024, 0.3, 1.0, 0.9, ptr(d["rscore"]), stream()))

    if args.trace_only:
        for m in SIZES:
            d = case(m)
            for _ in range(10):
                seeds(d), consensus(d), pose_score(d), ransac(d)
        torch.cuda.synchronize()
        return
    out = {"reps": args.reps, "inner": args.inner, "peak_i8_mac_per_second": PEAK_I8_MAC}
    line = lambda tag, s, more="": print(f"{tag:34s} {s[0]:11.2f} us ({s[1]:.2f} .. {s[2]:.2f}) {more}", flush=True)  # noqa: E731

    a = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    s = measure(lambda: b.copy_(a), inner=4)
    rate = 2.0 * a.numel() / (s[0] * 1e-6)
    out["copy_512MiB"] = {"us": s, "bytes_per_second_read_plus_write": rate}
    line("copy 512 MiB", s, f"{rate / 1e12:.2f} TB/s read + write")
    del a, b

    gp = sp.GlobalRegistrationParams(method="COMPATIBILITY", inlier_distance=0.3, min_edge=1.0)
    for m in SIZES:
        d = case(m)
        mp = (m + 127) // 128 * 128
        row = {}
        s = measure(lambda: seeds(d))
        mem, mfma = 2.0 * mp * mp / rate * 1e6, float(m) ** 3 / PEAK_I8_MAC * 1e6
        row["seeds"] = {"us": s, "memory_bound_us": mem, "mfma_bound_us": mfma, "fraction_of_memory_bound": mem / s[0],
                        "fraction_of_mfma_bound": mfma / s[0]}
        line(f"M = {m}: seeds", s, f"memory bound {mem:.2f} us ({100 * mem / s[0]:.1f} %), MFMA bound {mfma:.2f} us ({100 * mfma / s[0]:.1f} %)")
        row["consensus"] = {"us": measure(lambda: consensus(d))}
        line(f"M = {m}: consensus", row["consensus"]["us"])
        row["pose_score"] = {"us": measure(lambda: pose_score(d))}
        line(f"M = {m}: pose_score, 64 poses", row["pose_score"]["us"])
        seed_idx, cons = d["seed_idx"].cpu().numpy(), d["cons"].cpu().numpy()
        state = {}

        def host_part():
            state["p"] = sp.compat_poses(d["cs_host"], d["ct_host"], seed_idx, cons)
            sp.compat_select(np.arange(len(state["p"][0]), 0, -1).astype(np.int32), state["p"][0], state["p"][1], 64)

        row["host"] = {"us": wall(host_part), "poses": int(len(sp.compat_poses(d["cs_host"], d["ct_host"], seed_idx, cons)[0]))}
        line(f"M = {m}: host (poses, select)", row["host"]["us"], f"{row['host']['poses']} poses")
        row["guesses"] = {"us": wall(lambda: sp.compat_guesses(d["cs"], d["ct"], gp))}
        line(f"M = {m}: compat_guesses (wall)", row["guesses"]["us"])
        row["ransac_score_50000"] = {"us": measure(lambda: ransac(d))}
        line(f"M = {m}: ransac_score, 50 000", row["ransac_score_50000"]["us"])
        out[f"M_{m}"] = row
        del d
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
