"""sp_deskew_imu against sp_deskew_constant_velocity: 1 M points, each attribute set, a 26-row trajectory, 3 warm-ups and 20 launches
between HIP events; sp_imu_deskew_trajectory_host's host time for 26 and 300 samples. One JSON line."""
import ctypes as C
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sycl_points_amd import _lib  # noqa: E402

spec = importlib.util.spec_from_file_location("imu_cpu_helpers", os.path.join(ROOT, "tests", "test_imu_cpu.py"))
cpu = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cpu)
L = _lib.lib()
vp = C.c_void_p
N = 1_000_000
pts, covs, nrm = cpu.random_cloud(N)
t = np.sort(np.random.RandomState(1).uniform(0, 100, N)).astype(np.float32)  # a scan: stamps ascend with the index
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
P, Cv, Nr, T = dev(pts), dev(covs), dev(nrm), dev(t)
Po, Co, No = torch.empty_like(P), torch.empty_like(Cv), torch.empty_like(Nr)
traj = cpu.synthetic_trajectory(27, 1.5, 3.0, equal_pair=False)
rows = dev(cpu.lib_intervals(L, traj))
twist = np.array([0.05, 0.02, -0.03, 1.0, 0.5, -0.2], np.float32)
st = vp(torch.cuda.current_stream().cuda_stream)
ptr = lambda x: None if x is None else vp(x.data_ptr())  # noqa: E731
out = {}
for name, (wc, wn) in {"points": (0, 0), "points+normals": (0, 1), "points+covs": (1, 0), "all": (1, 1)}.items():
    c, co, n, no = (Cv if wc else None), (Co if wc else None), (Nr if wn else None), (No if wn else None)
    calls = {"imu": lambda: L.sp_deskew_imu(ptr(P), ptr(c), ptr(n), ptr(T), N, ptr(rows), 26, ptr(Po), ptr(co), ptr(no), st),
             "cv": lambda: L.sp_deskew_constant_velocity(ptr(P), ptr(c), ptr(n), ptr(T), N, twist.ctypes.data_as(vp), 0.1, ptr(Po),
                                                         ptr(co), ptr(no), st)}
    for which, fn in calls.items():
        for _ in range(3):
            assert fn() == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[f"{which}_{name}_us"] = round(e0.elapsed_time(e1) * 1e3 / 20, 2)
    out[f"ratio_{name}"] = round(out[f"imu_{name}_us"] / out[f"cv_{name}_us"], 3)
for rate, label in ((200, 26), (2950, 300)):
    ts, g, a = cpu.imu_samples(rate, 19.96, 0.2, seed=1)
    keep = slice(0, None)
    best = 1e9
    for _ in range(20):
        t0 = time.perf_counter()
        rc, status, tr = cpu.c_trajectory(L, ts[keep], g[keep], a[keep], 20.001, 0.1)
        best = min(best, time.perf_counter() - t0)
    out[f"trajectory_host_{label}_poses_us"] = round(best * 1e6, 1)
    out[f"trajectory_host_{label}_n_traj"] = int(len(tr))
print(json.dumps(out))
