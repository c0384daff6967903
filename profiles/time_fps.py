"""Farthest point sampling: every form of sp_internal_fps, and the CPU restatement of the reference operator, on the same
clouds in one process: one JSON line (also written to profiles/fps_timing.json).

Clouds: uniform in a 20 m cube (Mt19937Cloud, seed 1234) of 6 000, 16 384, 70 000 and 1 048 576 points; S = 1000 and 4096.
Per form: the median of 30 calls (after 3 of warm-up) timed by HIP events, its launch count and the time per sample. The
sweeps (S = 1000, median of 10): the persistent form's points per lane at 70 k and 1 M, and the per-sample form's grid
cap at 1 M. The per-sample form is the reference's shape (an update and an argmax per sample) kept on the device; the CPU restatement
(tests/cpp/fps_restate.cpp, g++ -O2, one call) is the reference's arithmetic on one host core without its host round trips.
Run from the repository root: python profiles/time_fps.py"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sycl_points_amd import _lib  # noqa: E402
from sycl_points_amd.synthetic import Mt19937Cloud  # noqa: E402

ONE_WG_CAP = 16384
PERSIST_CAP = 1 << 21


def restatement():
    so = os.path.join(tempfile.mkdtemp(), "libfps_restate.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "fps_restate.cpp"), "-o", so])
    R = C.CDLL(so)
    R.fps_restate.restype = None
    R.fps_restate.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    return R


def median_ms(fn, reps=30, warm=3):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    L = _lib.lib()
    torch.cuda.set_device(0)
    R = restatement()
    out = {"timing": "median of 30 C-ABI calls after 3 warm-up (HIP events); CPU restatement: one call, wall clock",
           "device": torch.cuda.get_device_name(0)}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n in (6000, ONE_WG_CAP, 70_000, 1_048_576):
        pts_np = Mt19937Cloud(1234).uniform_points(n, 10.0)
        P = torch.from_numpy(pts_np).cuda()
        flags = torch.empty(n, dtype=torch.uint8, device="cuda")
        d = torch.empty(n, dtype=torch.float32, device="cuda")
        for S in (1000, 4096):
            order = torch.empty(S, dtype=torch.int32, device="cuda")
            nb = L.sp_fps_workspace_bytes(n, S)
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
            row = {"points": n, "samples": S}
            ref_order = np.empty(S, np.uint32)
            ref_d = np.empty(n, np.float32)
            t0 = time.perf_counter()
            R.fps_restate(pts_np.ctypes.data_as(C.c_void_p), n, S, 0, ref_order.ctypes.data_as(C.c_void_p),
                          ref_d.ctypes.data_as(C.c_void_p))
            cpu_ms = (time.perf_counter() - t0) * 1e3
            row["cpu_restatement"] = {"ms": cpu_ms, "us_per_sample": cpu_ms * 1e3 / S}
            forms = (["one_workgroup"] if n <= ONE_WG_CAP else []) + ["persistent", "per_sample"]

            def call(code):
                _lib.check(L.sp_internal_fps(code, C.c_void_p(P.data_ptr()), n, S, 0, C.c_void_p(order.data_ptr()),
                                             C.c_void_p(flags.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(ws.data_ptr()),
                                             nb, stream))

            def timed(code, reps=30):
                ms = median_ms(lambda: call(code), reps=reps)
                _lib.check(L.sp_fps_status(C.c_void_p(ws.data_ptr()), stream))
                assert np.array_equal(order.cpu().numpy().view(np.uint32), ref_order), code
                return ms

            launches = {"one_workgroup": 1, "persistent": 2, "per_sample": S + 1}  # persistent: + the record reset
            for form in forms + ["auto"]:
                ms = timed(_lib.FPS_FORM[form])
                chosen = form if form != "auto" else ("one_workgroup" if n <= ONE_WG_CAP else "persistent")
                row[form] = {"ms": ms, "us_per_sample": ms * 1e3 / S, "launches": launches[chosen]}
            if S == 1000 and n > ONE_WG_CAP:
                row["persistent_points_per_lane"] = {
                    str(per): timed(_lib.FPS_FORM["persistent"] | (per << 8), reps=10) * 1e3 / S
                    for per in (1, 2, 4, 8) if -(-n // (1024 * per)) <= 256}
            if S == 1000 and n == 1_048_576:
                row["per_sample_grid_cap"] = {str(256 * c): timed(_lib.FPS_FORM["per_sample"] | (c << 8), reps=10) * 1e3 / S
                                              for c in (1, 4, 8, 16)}
            out[f"n{n}_s{S}"] = row
    line = json.dumps(out)
    with open(os.path.join(ROOT, "profiles", "fps_timing.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
