"""Voxelised GICP without a GPU: the engineered scene of tests/f64_voxel_registration.py holds its own conditions on the
oracle's VoxelHashMap (so that no case of tests/test_gpu_voxel_registration.py is ever decided by rounding), the float64 model's fast
path equals finite differences on the model's own correspondences, and sp_vhm_neighbor_offsets_host (host code of the library) gives
the probing order the header states."""
import ctypes as C

import numpy as np
import pytest

import f64_factors as f64
import f64_voxel_registration as vr


@pytest.fixture(scope="module")
def scene():
    return vr.build_scene()


@pytest.fixture(scope="module")
def export(orc, scene):
    m = orc.voxel_hash_map(vr.VOXEL_SIZE)
    m.set("min_num_point", vr.MIN_NUM_POINT)
    m.add_point_cloud(scene["tgt"], covs=scene["tcov"])
    r = m.downsampling(distance=1e7)
    return vr.Export(r["points"], r["covs"], r["keys"])


def test_scene_conditions_hold_for_the_fixed_seed(scene, export):
    bad, counts = vr.scene_report(scene, export)
    print("\n[voxel registration scene]", len(scene["tgt"]), "target points in", len(scene["counts"]), "cells,", len(export.keys),
          "exported;", len(scene["src"]), "source points;", counts)
    assert not bad, bad[:10]
    assert 55 <= len(scene["counts"]) <= 65 and 280 <= len(scene["src"]) <= 320
    assert all(1 <= m <= 5 for m in scene["counts"].values())
    assert abs(np.linalg.norm((scene["T_trial"] - scene["T"])[:3, 3]) - 0.6) < 1e-6


@pytest.mark.parametrize("mode", [1, 7, 27])
def test_trial_pose_moves_at_least_half_of_the_correspondences(scene, export, mode):
    nn, _, keys = vr.correspondences(export, scene["src"], scene["T"], mode)
    _, _, fresh = vr.correspondences(export, scene["src"], scene["T_trial"], mode)
    inl = nn >= 0
    assert inl.sum() >= 100
    assert (fresh[inl] != keys[inl]).mean() >= 0.5, (mode, (fresh[inl] != keys[inl]).mean())


def test_more_cells_never_lose_a_correspondence(scene, export):
    n = {mode: (vr.correspondences(export, scene["src"], scene["T"], mode)[0] >= 0) for mode in (1, 7, 27)}
    assert (n[7] | ~n[1]).all() and (n[27] | ~n[7]).all()
    assert n[1].sum() < n[7].sum() < n[27].sum()  # the face and the edge / corner classes are really reached


@pytest.mark.parametrize("factor", ["GICP", "POINT_TO_DISTRIBUTION"])
@pytest.mark.parametrize("mode", [1, 7, 27])
def test_model_fast_path_equals_finite_differences(scene, export, mode, factor):
    nn, d2, _ = vr.correspondences(export, scene["src"], scene["T"], mode)
    case = vr.case_for(export, scene["src"], scene["scov"], scene["T"], nn, d2)
    s = vr.robust_scale(case, factor)
    for loss in ("NONE", "GEMAN_MCCLURE"):
        a = f64.system_fd(case, factor, loss, s)
        b = f64.system_fast(case, factor, loss, s)
        d = f64.distances(b["H"], b["b"], b["error"], a)
        assert max(d.values()) <= 1e-6, (mode, factor, loss, d)  # the bound of tests/test_oracle_factors_f64.py
        assert a["inlier"] == b["inlier"] == int((nn >= 0).sum())


def test_probing_order():
    from sycl_points_amd import _lib

    L = _lib.lib()
    got = {}
    for n in (1, 7, 27):
        out = np.full(3 * 27 + 3, 77, np.int32)
        assert L.sp_vhm_neighbor_offsets_host(n, out.ctypes.data_as(C.c_void_p)) == _lib.SP_OK
        assert (out[3 * n:] == 77).all()
        got[n] = [tuple(int(v) for v in out[3 * j:3 * j + 3]) for j in range(n)]
        assert len(set(got[n])) == n and got[n][0] == (0, 0, 0)
        assert set(got[n]) == set(vr.offsets(n))
    assert got[27][:7] == got[7] and got[7][:1] == got[1]
    out = np.full(81, 77, np.int32)
    for n in (0, 5, 6, 8, 26, 28, -1):
        assert L.sp_vhm_neighbor_offsets_host(n, out.ctypes.data_as(C.c_void_p)) == _lib.SP_ERR_INVALID_ARGUMENT
        assert b"neighbor_voxels must be 1, 7 or 27" in L.sp_last_error()
        assert (out == 77).all()
    assert L.sp_vhm_neighbor_offsets_host(7, None) == _lib.SP_ERR_INVALID_ARGUMENT


def test_kernels_use_no_scratch():
    """The build keeps the compiler's resource report of csrc/voxel_registration.hip: the 27-cell linearisation holds 27 first keys
    and their slots per lane next to the 28 sums, and nothing of any kernel of the unit may go to scratch."""
    import os
    import re

    from sycl_points_amd import _lib

    _lib.build()
    report = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "lib", "voxel_registration.resources.txt")
    rows = [l for l in open(report) if "vhm_" in l]
    assert len([l for l in rows if "vhm_linearize_kernel" in l]) == 5 * 2 * 3 and len([l for l in rows if "vhm_error_kernel" in l]) == 5 * 2
    for row in rows:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", row).group(1)) == 0, row
        assert int(re.search(r"VGPRs Spill: (\d+)", row).group(1)) == 0, row
        assert int(re.search(r"VGPRs: (\d+)", row).group(1)) <= 168, row
