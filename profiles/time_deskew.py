"""Constant-velocity deskew: every instantiation of the kernel (points; + covs; + normals; all three) on 1 000 000 points, 20
calls each after 3 of warm-up, out of place. Meant to run under `rocprofv3 --kernel-trace --stats -- python
profiles/time_deskew.py`, whose per-kernel statistics are the figures DESIGN.md quotes; by itself it prints the HIP-event
medians as one JSON line. Run from the repository root."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sycl_points_amd import _lib  # noqa: E402

BYTES = {"points": 36, "points+normals": 68, "points+covs": 148, "all": 180}


def main():
    L = _lib.lib()
    torch.cuda.set_device(0)
    n = 1_000_000
    g = torch.Generator(device="cuda").manual_seed(1234)
    pts = torch.rand((n, 4), device="cuda", generator=g) * 100 - 50
    covs = torch.rand((n, 16), device="cuda", generator=g)
    nrm = torch.rand((n, 4), device="cuda", generator=g)
    t = torch.rand(n, device="cuda", generator=g) * 100
    po, co, no = torch.empty_like(pts), torch.empty_like(covs), torch.empty_like(nrm)
    tw = np.array([0.01, -0.015, 0.05, 1.4, 0.5, -0.1], np.float32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    out = {"n": n, "device": torch.cuda.get_device_name(0), "timing": "median of 20 calls after 3 warm-up (HIP events)"}
    for name, (c, m) in {"points": (0, 0), "points+normals": (0, 1), "points+covs": (1, 0), "all": (1, 1)}.items():
        def call():
            rc = L.sp_deskew_constant_velocity(p(pts), p(covs) if c else None, p(nrm) if m else None, p(t), n,
                                               tw.ctypes.data_as(C.c_void_p), 0.1, p(po), p(co) if c else None,
                                               p(no) if m else None, st)
            assert rc == 0
        for _ in range(3):
            call()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
        for a, b in ev:
            a.record()
            call()
            b.record()
        torch.cuda.synchronize()
        us = float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3
        out[name] = {"bytes_per_point": BYTES[name], "event_us": round(us, 2), "TB_per_s": round(BYTES[name] * n / us * 1e-6, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
