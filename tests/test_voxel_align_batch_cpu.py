"""sp_vhm_align_batch (csrc/voxel_registration_batch.hip) without a GPU: the workspace size, argument errors that need no device,
and the compiler's resource report of the new kernels — every instantiation without scratch memory and without a spilled
register, within the registers a lane of its workgroup size has (128 at 1024 lanes, 256 at 512 and 256)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_POINTS, MAX_BATCH = 16384, 65535  # SP_VHM_ALIGN_BATCH_MAX_POINTS, SP_ALIGN_BATCH_MAX


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


def test_workspace_bytes(L):
    f = L.sp_vhm_align_batch_workspace_bytes
    ns, bs = (1, 2, 64, 257, 513, 1025, MAX_POINTS), (1, 2, 3, 257, 4096, MAX_BATCH)
    for n in ns:
        for b in bs:
            assert f(n, b) >= 32 * n + 4 * n * b, (n, b)
    for b in bs:  # strictly monotone in n ...
        vals = [f(n, b) for n in ns]
        assert vals == sorted(vals) and len(set(vals)) == len(vals), (b, vals)
    for n in ns:  # ... and in batch
        vals = [f(n, b) for b in bs]
        assert vals == sorted(vals) and len(set(vals)) == len(vals), (n, vals)
    for n, b in ((0, 4), (MAX_POINTS + 1, 4), (900, 0), (900, MAX_BATCH + 1)):
        assert f(n, b) == 0, (n, b)


def call(L, _lib, **kw):
    """sp_vhm_align_batch with made-up non-null pointers that a failing call never follows (there is no device here)"""
    fp, op = _lib.FactorParams(), _lib.OptParams()
    fp.reg_type = kw.get("reg_type", 3)  # SP_REG_GICP
    op.method, op.max_iterations = kw.get("method", 0), kw.get("max_iterations", 10)
    sc = (C.c_float * 1)(1.0)
    p = C.c_void_p(4096)
    args = dict(map=p, src=p, covs=p, n=100, T_in=p, T_out=p, batch=4, fp=C.byref(fp), op=C.byref(op), sc=sc, n_levels=1, cells=1,
                results=p, keys=None, ws=p, ws_bytes=1 << 30)
    args.update({k: v for k, v in kw.items() if k in args})
    return L.sp_vhm_align_batch(args["map"], args["src"], args["covs"], args["n"], args["T_in"], args["T_out"], args["batch"], args["fp"],
                                args["op"], args["sc"], args["n_levels"], args["cells"], args["results"], args["keys"], args["ws"],
                                args["ws_bytes"], None)


def test_argument_errors_need_no_device(L):
    from sycl_points_amd import _lib

    bad = _lib.SP_ERR_INVALID_ARGUMENT
    for name in ("map", "src", "T_in", "T_out", "fp", "op", "sc", "results"):
        assert call(L, _lib, **{name: None}) == bad, name
        assert b"[sp_vhm_align_batch] null argument" in L.sp_last_error(), name
    for levels in (0, 9, -1):
        assert call(L, _lib, n_levels=levels) == bad
        assert b"n_levels must be in 1..SP_OPT_MAX_LEVELS" in L.sp_last_error()
    assert call(L, _lib, method=7) == bad and b"unknown optimization method" in L.sp_last_error()
    for it in (0, 65536, -3):
        assert call(L, _lib, max_iterations=it) == bad and b"max_iterations must be in 1..65535" in L.sp_last_error()
    assert call(L, _lib, reg_type=0) == bad and b"reg_type must be GICP or POINT_TO_DISTRIBUTION" in L.sp_last_error()


def rows_of(report):
    out = {}
    for line in open(report):
        m = re.search(r"vhm_optimize_batch_kernelILi(\d)ELb([01])ELi(\d+)ELi(\d+)EE", line)
        if m:
            key = tuple(int(m.group(i)) for i in (1, 2, 3, 4))  # loss, point-to-distribution, cells, lanes
            out[key] = tuple(int(re.search(pat + r" (\d+)", line).group(1))
                             for pat in (r"VGPRs:", r"ScratchSize \[bytes/lane\]:", r"VGPRs Spill:"))
    return out


def test_resource_report_of_the_batch_kernels(L):
    rows = rows_of(os.path.join(ROOT, "sycl_points_amd", "lib", "voxel_registration_batch.resources.txt"))
    lanes_of = {}
    for (loss, p2d, cells, lanes), (vgprs, scratch, spills) in sorted(rows.items()):
        assert scratch == 0 and spills == 0, (loss, p2d, cells, lanes, scratch, spills)
        assert vgprs <= {1024: 128, 512: 256, 256: 256}[lanes], (loss, p2d, cells, lanes, vgprs)
        lanes_of.setdefault(cells, set()).add(lanes)
    # loss x factor x cells x (256 lanes | the table's workgroup size of that cell count)
    assert set(lanes_of) == {1, 7, 27} and all(256 in v and len(v) == 2 for v in lanes_of.values()), lanes_of
    assert len(rows) == 5 * 2 * 3 * 2, sorted(rows)
