"""Weighted random sampling: the device path of PreprocessFilter::weighted_random_sampling against the CPU restatement's host
loop, on weights that start on the device: one JSON line (also written to profiles/sampling_timing.json).

Per size (69 088: the golden target scan with its intensities as weights; 1 048 576: U(0, 1) weights with a fifth of zeros),
m = 1000:
  device   sp_weight_check + its 8-byte read-back, the host's draws (one per positive weight, std::mt19937 through the
           restatement's export), their upload (4 B per positive weight) and sp_weighted_sample_flags: wall clock of the whole
           sequence, the median of 20 after 3 of warm-up; the C-ABI calls alone by HIP events beside it.
  host     what the facade would otherwise do: the N weights copied to the host (4 B per point), the restatement's loop (a
           log, a draw and a heap step per positive weight), the N flags copied back (1 B per point): wall clock, median of 5.
This is the C-ABI sequence with preallocated buffers and pinned staging memory, not the C++ facade
(PreprocessFilter::weighted_random_sampling keeps its draws in pageable memory, takes its scratch per call and goes on to move
the rows): the facade has not been timed.
`--once N` runs the device sequence a few times on N points and exits (for a kernel trace).
Run from the repository root: python profiles/time_sampling.py"""
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

M = 1000


def build_restatement(out_dir):
    so = os.path.join(out_dir, "libsampling_restate.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "sampling_restate.cpp"), "-o", so])
    R = C.CDLL(so)
    R.sampling_weighted_restate.restype = C.c_int
    R.sampling_weighted_restate.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    R.sampling_draws.restype = None
    R.sampling_draws.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p]
    return R


def weights_for(n):
    if n == 69_088:  # the golden target scan: x, y, z, scalar_intensity as little-endian floats
        raw = open(os.path.join(ROOT, "tests", "golden", "target.ply"), "rb").read()
        body = raw.split(b"end_header\n", 1)[1]
        return np.ascontiguousarray(np.frombuffer(body, dtype="<f4", count=n * 4).reshape(n, 4)[:, 3])
    rs = np.random.RandomState(1)
    w = rs.uniform(0.0, 1.0, n).astype(np.float32)
    w[rs.uniform(size=n) < 0.2] = 0.0
    return w


class DevicePath:
    def __init__(self, L, R, w_np):
        self.L, self.R, self.n = L, R, len(w_np)
        self.w = torch.from_numpy(w_np).cuda()
        self.report = torch.empty(2, dtype=torch.int32, device="cuda")
        self.report_host = torch.empty(2, dtype=torch.int32).pin_memory()
        self.u_host = torch.empty(self.n, dtype=torch.float32).pin_memory()
        self.u = torch.empty(self.n, dtype=torch.float32, device="cuda")
        self.flags = torch.empty(self.n, dtype=torch.uint8, device="cuda")
        self.nb = L.sp_weighted_sample_workspace_bytes(self.n)
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device="cuda")
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.positive = int((w_np > 0).sum())

    def check(self):
        assert self.L.sp_weight_check(C.c_void_p(self.w.data_ptr()), self.n, C.c_void_p(self.report.data_ptr()), self.st) == 0

    def select(self):
        assert self.L.sp_weighted_sample_flags(C.c_void_p(self.w.data_ptr()), C.c_void_p(self.u.data_ptr()), self.n, M,
                                               C.c_void_p(self.flags.data_ptr()), None, C.c_void_p(self.ws.data_ptr()), self.nb,
                                               self.st) == 0

    def whole(self):
        self.check()
        self.report_host.copy_(self.report, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        positive = int(self.report_host[0])
        self.R.sampling_draws(1234, positive, C.c_void_p(self.u_host.data_ptr()))
        self.u[:positive].copy_(self.u_host[:positive], non_blocking=True)
        self.select()
        torch.cuda.current_stream().synchronize()


def events_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def wall_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    L = _lib.lib()
    torch.cuda.set_device(0)
    R = build_restatement(tempfile.mkdtemp())
    if len(sys.argv) > 2 and sys.argv[1] == "--once":
        d = DevicePath(L, R, weights_for(int(sys.argv[2])))
        for _ in range(5):
            d.whole()
        return
    out = {"timing": "wall clock, median (device and draws: 20 after 3 warm-up; host loop: 5 after 1); *_events_ms: HIP events "
                     "around the C-ABI call alone; the C-ABI sequence, not the C++ facade", "device": torch.cuda.get_device_name(0), "m": M}
    for n in (69_088, 1_048_576):
        w_np = weights_for(n)
        d = DevicePath(L, R, w_np)
        d.whole()
        flags_host = np.empty(n, np.uint8)
        flags_dev = torch.empty(n, dtype=torch.uint8, device="cuda")

        def host_loop():
            w_host = d.w.cpu().numpy()
            rc = R.sampling_weighted_restate(1234, w_host.ctypes.data_as(C.c_void_p), n, M, flags_host.ctypes.data_as(C.c_void_p))
            assert rc == 0
            flags_dev.copy_(torch.from_numpy(flags_host))
            torch.cuda.synchronize()

        row = {"positive": d.positive, "device_wall_ms": wall_ms(d.whole, 20, 3), "check_events_ms": events_ms(d.check),
               "select_events_ms": events_ms(d.select), "host_loop_wall_ms": wall_ms(host_loop, 5, 1)}
        row["draws_wall_ms"] = wall_ms(lambda: R.sampling_draws(1234, d.positive, C.c_void_p(d.u_host.data_ptr())), 20, 3)
        row["same_flags"] = bool(np.array_equal(d.flags.cpu().numpy(), flags_host))
        out[str(n)] = row
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, "profiles", "sampling_timing.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
