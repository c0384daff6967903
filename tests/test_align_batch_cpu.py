"""sp_gicp_align_batch / sp_align_best_host (csrc/registration_batch.hip) without a GPU: the workspace size, the rule that picks the
best hypothesis, argument errors that need no device, and the compiler's resource report of the new kernels — every 1024-lane
instantiation within the 128 registers such a workgroup has, and spilling no more of them than the same
<LOSS, FAST_NN, P2D, 1024> lane-per-point instantiation of gicp_optimize_kernel in registration_opt.resources.txt (the same
build, the same point loops)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_POINTS, MAX_BATCH = 16384, 65535  # SP_ALIGN_BATCH_MAX_POINTS, SP_ALIGN_BATCH_MAX


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


def test_workspace_bytes(L):
    f = L.sp_gicp_align_batch_workspace_bytes
    ns, bs = (1, 64, 900, 1025, MAX_POINTS), (1, 2, 257, 4096, MAX_BATCH)
    for n in ns:
        for b in bs:
            assert f(n, b) >= b * 48 * n, (n, b)
    for b in bs:  # monotone in n ...
        vals = [f(n, b) for n in ns]
        assert vals == sorted(vals) and len(set(vals)) == len(vals)
    for n in ns:  # ... and in batch
        vals = [f(n, b) for b in bs]
        assert vals == sorted(vals) and len(set(vals)) == len(vals)
    for n, b in ((0, 4), (MAX_POINTS + 1, 4), (900, 0), (900, MAX_BATCH + 1)):
        assert f(n, b) == 0, (n, b)


def block(_lib, inlier, error, status=0, T=None):
    r = _lib.AlignResult()
    r.T[:] = T if T is not None else [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    r.inlier, r.error, r.status = inlier, error, status
    return r


def best(L, _lib, blocks):
    arr = (_lib.AlignResult * max(len(blocks), 1))(*blocks)
    out = C.c_size_t(12345)
    assert L.sp_align_best_host(C.byref(arr), len(blocks), C.byref(out)) == _lib.SP_OK
    return out.value


def test_best_host_rule(L):
    from sycl_points_amd import _lib

    nan_pose = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, float("nan"), 0, 0, 1]
    inf_pose = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, float("inf"), 0, 1]
    # the most inliers wins
    assert best(L, _lib, [block(_lib, 10, 1.0), block(_lib, 30, 9.0), block(_lib, 20, 0.1)]) == 1
    # ties: the smaller error, then the lower index
    assert best(L, _lib, [block(_lib, 30, 2.0), block(_lib, 30, 1.0), block(_lib, 30, 1.5)]) == 1
    assert best(L, _lib, [block(_lib, 5, 3.0), block(_lib, 30, 1.0), block(_lib, 30, 1.0)]) == 1
    assert best(L, _lib, [block(_lib, 30, 1.0), block(_lib, 30, 1.0)]) == 0
    # skipped: a wait that ran out (status 2), a pose that is not finite, an error that is not finite, no inlier
    bad = [block(_lib, 99, 0.1, status=2), block(_lib, 98, 0.1, T=nan_pose), block(_lib, 97, 0.1, T=inf_pose),
           block(_lib, 96, float("nan")), block(_lib, 95, float("inf")), block(_lib, 0, 0.0)]
    assert best(L, _lib, bad + [block(_lib, 3, 7.0)]) == len(bad)
    assert best(L, _lib, [block(_lib, 3, 7.0)] + bad) == 0
    # nothing qualifies: best == batch
    assert best(L, _lib, bad) == len(bad)
    assert best(L, _lib, []) == 0
    assert L.sp_align_best_host(None, 3, C.byref(C.c_size_t())) == _lib.SP_ERR_INVALID_ARGUMENT
    arr = (_lib.AlignResult * 1)(block(_lib, 1, 1.0))
    assert L.sp_align_best_host(C.byref(arr), 1, None) == _lib.SP_ERR_INVALID_ARGUMENT


def test_null_arguments_need_no_device(L):
    from sycl_points_amd import _lib

    fp, op, sc = _lib.FactorParams(), _lib.OptParams(), (C.c_float * 1)(1.0)
    rc = L.sp_gicp_align_batch(None, None, None, None, 4, C.byref(fp), C.byref(op), sc, 1, None, None, 0, None)
    assert rc == _lib.SP_ERR_INVALID_ARGUMENT
    assert b"sp_gicp_align_batch" in L.sp_last_error()


def test_python_best_of_is_the_library_rule(L):
    import numpy as np

    import sycl_points_amd.api as sp

    def res(inlier, error, tx=0.0):
        r = sp.RegistrationResult()
        r.T = np.eye(4, dtype=np.float32)
        r.T[0, 3] = tx
        r.inlier, r.error = inlier, error
        return r

    assert sp.Registration.best_of([res(10, 1.0), res(30, 2.0), res(30, 1.0), res(40, 1.0, float("nan"))]) == 2
    assert sp.Registration.best_of([res(0, 0.0), res(0, 0.0)]) == 2
    assert sp.Registration.best_of([]) == 0


def rows_of(report, kernel):
    out = {}
    for line in open(report):
        m = re.search(kernel + r"ILi(\d)ELb([01])ELb([01])ELi(\d+)E(Lb([01])E)?E", line)
        if m:
            key = (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(6) or 0))
            out[key] = (int(re.search(r"VGPRs: (\d+)", line).group(1)), int(re.search(r"VGPRs Spill: (\d+)", line).group(1)))
    return out


def test_resource_report_of_the_batch_kernels(L):
    lib = os.path.join(ROOT, "sycl_points_amd", "lib")
    batch = rows_of(os.path.join(lib, "registration_batch.resources.txt"), "gicp_optimize_batch_kernel")
    single = rows_of(os.path.join(lib, "registration_opt.resources.txt"), "gicp_optimize_kernel")
    assert len(batch) == 5 * 2 * 2 * 2, sorted(batch)  # loss x search form x factor x (256 | 1024 lanes)
    for (loss, fast, p2d, lanes, _), (vgprs, spills) in sorted(batch.items()):
        assert vgprs <= (128 if lanes == 1024 else 256), (loss, fast, p2d, lanes, vgprs)
        if lanes == 1024:
            yardstick = single[(loss, fast, p2d, 1024, 0)][1]  # lane per point (not the wave-per-point form)
            assert spills <= yardstick, (loss, fast, p2d, spills, yardstick)
        else:
            assert spills == 0, (loss, fast, p2d, spills)
