"""VoxelHashMap on the GPU (csrc/voxel_hash_map.hip over csrc/sp_voxel_table.h) on engineered probe chains and hot voxels: the
scenarios of tests/voxel_chains.py, which tests/test_voxel_chains_cpu.py runs on the oracle alone, with the device map first in the
list. Voxel 1.0, identity pose. What they hold the device to, all of it exactly:
  * the probe limit: of 150 keys on one probe sequence 100 get in, at 30 029 and at 60 013 slots, in one frame (150 lanes racing
    their swaps along one sequence) and one per frame (the model's slot layout, key by key);
  * 64 keys that share only their first slot, in one frame: none is lost to the race on that slot;
  * a chain cut by stale removal: the keys behind the cut are out of a lookup's reach, the next insert claims the cut slot and the
    table holds one key twice, the lookup answers from the entry in front, the rehash merges the two by adding;
  * 8192 points of one frame in one voxel or seven: counts exact, sums bit-equal to float64 (dyadic inputs: exact in any order);
  * 512 equal covariances per voxel against that covariance in float64: E_dev <= 4 x E_ref + 1e-6, E_ref the oracle's error on the
    same input; both printed (-s); the measured figures are in DESIGN.md 2.3."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


vc = load("voxel_chains")


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


@pytest.fixture(scope="module")
def helpers():
    return load("test_gpu_voxel_hash_map")  # cloud()


class DevVhm:
    """api.VoxelHashMap behind the interface the scenarios drive"""

    def __init__(self, sp, cloud, voxel):
        self.sp, self.cloud, self.m = sp, cloud, sp.VoxelHashMap(voxel)

    def set(self, name, value):
        self.m._set(name, value)

    def info(self, name):
        return self.m.info(name)

    def add(self, pts, covs=None, rgb=None, intensities=None):
        self.m.add_point_cloud(self.cloud(self.sp, pts, covs, rgb, intensities) if len(pts) else self.sp.PointCloudShared())

    def overlap(self, pts):
        return self.m.compute_overlap_ratio(self.cloud(self.sp, pts))

    def rows(self):
        r = self.m.downsampling(distance=1e7)
        host = lambda t, has: t.cpu().numpy() if has else None  # noqa: E731
        return {"keys": r.voxel_keys.cpu().numpy().view(np.uint64), "points": r.points.cpu().numpy().reshape(-1, 4),
                "covs": host(r.covs, r.has_cov()), "rgb": host(r.rgb, r.has_rgb()),
                "intensities": host(r.intensities, r.has_intensity())}


@pytest.fixture
def maps(sp, orc, helpers):
    """the device map, then the oracle: every scenario checks each of them against the model and the stated values"""
    return [DevVhm(sp, helpers.cloud, 1.0), vc.OracleVhm(orc, 1.0)]


@pytest.mark.parametrize("cap", [30029, 60013])
def test_probe_limit_one_frame(maps, cap):
    vc.vhm_probe_limit_one_frame(maps, cap)


def test_probe_limit_one_key_per_frame(maps):
    vc.vhm_probe_limit_one_per_frame(maps)


def test_diverging_chains(maps):
    vc.vhm_diverging(maps)


def test_cut_chain_duplicate_merge(maps):
    vc.vhm_cut_chain(maps)


@pytest.mark.parametrize("layout", list(vc.HOT_COUNTS))
def test_hot_voxels(maps, layout):
    vc.vhm_hot_voxels(maps, vc.HOT_COUNTS[layout])


def test_hot_covariances(maps):
    E_dev, E_ref = (vc.vhm_hot_covariances(m) for m in maps)
    print(f"VoxelHashMap, 512 equal covariances per voxel: E_dev = {E_dev:.3e}  E_ref = {E_ref:.3e}  "
          f"bound = 4 x E_ref + 1e-6 = {4 * E_ref + 1e-6:.3e}")
    assert E_dev <= 4 * E_ref + 1e-6, (E_dev, E_ref)
