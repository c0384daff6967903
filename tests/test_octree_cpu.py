"""sp_octree_* without a device: the argument checks of sp_octree_search come before any device work and sp_last_error() names
the argument. (tests/test_cabi.py holds the header, the exports and _lib.SIGNATURES together and the ABI at 7.)"""
import ctypes as C

import numpy as np


def test_search_argument_errors_without_gpu():
    from sycl_points_amd import _lib

    L = _lib.lib()
    q = np.zeros((4, 4), np.float32)
    idx, d2 = np.zeros((4, 101), np.int32), np.zeros((4, 101), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    # an empty tree needs no device: sp_octree_create with n == 0 only makes the handle
    h = C.c_void_p()
    assert L.sp_octree_create(None, 0, 0.1, 32, None, C.byref(h)) == _lib.SP_OK and h.value
    try:
        assert L.sp_octree_size(h) == 0
        nodes = C.c_uint64(7)
        assert L.sp_octree_info(h, 0, C.byref(nodes)) == _lib.SP_OK and nodes.value == 0
        assert L.sp_octree_search(h, vp(q), 4, 101, None, 0, vp(idx), vp(d2), None) == _lib.SP_ERR_INVALID_ARGUMENT
        assert b"`k`" in L.sp_last_error() and b"100" in L.sp_last_error()
        assert L.sp_octree_search(None, vp(q), 4, 5, None, 0, vp(idx), vp(d2), None) == _lib.SP_ERR_INVALID_ARGUMENT
        assert b"`octree`" in L.sp_last_error()
        assert L.sp_octree_search(h, vp(q), 4, 5, None, 0, None, vp(d2), None) == _lib.SP_ERR_INVALID_ARGUMENT
        assert b"`idx_out`" in L.sp_last_error()
        assert L.sp_octree_search(h, vp(q), 4, 5, None, 0, vp(idx), None, None) == _lib.SP_ERR_INVALID_ARGUMENT
        assert b"`d2_out`" in L.sp_last_error()
        assert L.sp_octree_search(h, None, 4, 5, None, 0, vp(idx), vp(d2), None) == _lib.SP_ERR_INVALID_ARGUMENT
        assert b"`queries`" in L.sp_last_error()
        assert not idx.any() and not d2.any()
        # nothing to search: no device work, SP_OK
        assert L.sp_octree_search(h, vp(q), 0, 5, None, 0, vp(idx), vp(d2), None) == _lib.SP_OK
        assert L.sp_octree_search(h, vp(q), 4, 0, None, 0, None, None, None) == _lib.SP_OK
        # removal on the empty tree: the id range is empty
        assert L.sp_octree_remove_by_flags(h, vp(np.ones(3, np.uint8)), vp(np.zeros(3, np.int32)), 3, None) == _lib.SP_ERR_RUNTIME
        assert b"identifier range" in L.sp_last_error()
        assert L.sp_octree_remove_by_flags(h, None, None, 0, None) == _lib.SP_OK
        assert L.sp_octree_export(h, None, None, None) == _lib.SP_OK
        assert L.sp_octree_info(h, 99, C.byref(nodes)) == _lib.SP_ERR_INVALID_ARGUMENT
    finally:
        L.sp_octree_destroy(h)
    assert L.sp_octree_create(None, 5, 0.1, 32, None, C.byref(h)) == _lib.SP_ERR_INVALID_ARGUMENT
    assert b"`points`" in L.sp_last_error()
