"""OccupancyGridMap on the GPU (csrc/occupancy_grid_map.hip over csrc/sp_voxel_table.h) on engineered probe chains and hot voxels:
the scenarios of tests/voxel_chains.py, which tests/test_voxel_chains_cpu.py runs on the restatement alone, with the device map first
in the list. Voxel 0.5, identity pose, carving off wherever a chain is fed (its points lie up to 5e5 m out). What they hold the
device to, all of it exactly:
  * the probe limit: of 130 keys on one probe sequence 128 get in, in one frame and one per frame (the model's slot layout);
  * 64 keys that share only their first slot, in one frame: none is lost to the race on that slot;
  * tombstones: lookups step over a `deleted` slot, a hit claims it before it reaches its own key further along, the table then
    holds that key twice and answers from the entry in front; the rehash keeps both entries;
  * 8192 points of one frame in one voxel or seven: hit_count exact, the sums of export() bit-equal to float64, log-odds the
    restatement's;
  * 4096 rays through the same five free cells: every miss counted.
Rows are compared as sorted (key, hit_count) pairs or in slot order, never through compare_state, which wants unique keys."""
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
def cpu():
    return load("test_occupancy_grid_cpu")  # RestatedMap, build_restatement


@pytest.fixture(scope="module")
def gpu():
    return load("test_gpu_occupancy_grid")  # DevMap


@pytest.fixture(scope="module")
def R(cpu, tmp_path_factory):
    return cpu.build_restatement(tmp_path_factory.mktemp("ogm_gpu_chains"))


@pytest.fixture
def maps(sp, cpu, gpu, R):
    """the device map, then the restatement: every scenario checks each of them against the model and the stated values"""
    return [gpu.DevMap(sp, vc.OGM_VOXEL), cpu.RestatedMap(R, vc.OGM_VOXEL)]


def test_probe_limit_one_frame(maps):
    vc.ogm_probe_limit_one_frame(maps)


def test_probe_limit_one_key_per_frame(maps):
    vc.ogm_probe_limit_one_per_frame(maps)


def test_diverging_chains(maps):
    vc.ogm_diverging(maps)


def test_tombstones_and_duplicate(maps):
    dev, ref = vc.ogm_tombstones(maps)
    assert dev == ref  # every voxel_probability and overlap ratio on the way: the restatement's, bit for bit


@pytest.mark.parametrize("layout", list(vc.HOT_COUNTS))
def test_hot_voxels(maps, layout):
    dev, ref = vc.ogm_hot_voxels(maps, vc.HOT_COUNTS[layout])
    assert np.array_equal(dev, ref)


def test_hot_voxels_with_carving(maps):
    dev, ref = vc.ogm_hot_carving(maps)
    for name in ("keys", "hit_count", "miss_count", "log_odds", "last_updated", "sum_xyz"):
        assert np.array_equal(dev[name], ref[name]), name
