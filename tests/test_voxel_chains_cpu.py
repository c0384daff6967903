"""The engineered chains and hot voxels of tests/voxel_chains.py on the CPU references alone: the oracle's VoxelHashMap, the
restatement of OccupancyGridMap and the Python TableModel agree on every scenario the GPU tests run, and the inputs produce the counts
those tests state. The GPU tests (tests/test_gpu_voxel_hash_map_chains.py, tests/test_gpu_occupancy_grid_chains.py) call the same
scenario functions with the device map in the list."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


vc = load("voxel_chains")


@pytest.fixture(scope="module")
def cpu():
    return load("test_occupancy_grid_cpu")


@pytest.fixture(scope="module")
def R(cpu, tmp_path_factory):
    return cpu.build_restatement(tmp_path_factory.mktemp("ogm_chains"))


@pytest.fixture
def vhm(orc):
    return [vc.OracleVhm(orc, 1.0)]


@pytest.fixture
def ogm(cpu, R):
    return [cpu.RestatedMap(R, vc.OGM_VOXEL)]


# ----------------------------------------------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("cap", [30029, 60013])
def test_chain_properties(cap):
    base = vc.BASE[cap]
    same = vc.chain(cap, 150, True, base)
    assert same[0] == base and same[1] - same[0] == cap * (cap - 2) and max(same) < 1 << 63
    if cap == 30029:
        assert same[1] - same[0] == 901680783
    sequence = [vc.slot_id(base, p, cap) for p in range(128)]
    assert len(set(sequence)) == 128  # cap is prime: a sequence meets no slot twice
    for k in same:
        assert [vc.slot_id(k, p, cap) for p in range(128)] == sequence
    apart = vc.chain(cap, 64, False, base)
    assert apart[0] == base and {vc.slot_id(k, 0, cap) for k in apart} == {sequence[0]}
    assert len({vc.slot_id(k, 1, cap) for k in apart}) == 64 and len({vc.stride(k, cap) for k in apart}) == 64
    if cap == 30029:
        assert sequence[0] == 20306 and [vc.slot_id(k, 1, cap) for k in apart[:3]] == [16939, 16937, 16935]


def test_neighbouring_chain():
    keys = vc.chain(30029, 3, True, vc.NEIGHBOURS)
    for k in keys:
        assert [vc.slot_id(k, p, 30029) for p in range(4)] == [6410, 6411, 6412, 6413]  # lanes 10 .. 13 of one wave


def test_key_to_point_to_key(orc, cpu, R):
    """every chain key survives key -> point at the cell's centre -> the map's own key arithmetic, in both maps"""
    keys = (vc.chain(30029, 150, True, vc.BASE[30029]) + vc.chain(60013, 150, True, vc.BASE[60013])
            + vc.chain(30029, 64, False, vc.BASE[30029]) + vc.chain(30029, 3, True, vc.NEIGHBOURS))
    for frac in (0.5, 0.25):
        pts = vc.points_of(keys, vc.OGM_VOXEL, frac)
        assert np.abs(pts[:, :3]).max() < 2 ** 19
        assert [int(k) for k in cpu.RestatedMap(R, vc.OGM_VOXEL).point_keys(pts)] == keys
    pts = vc.points_of(keys, 1.0)
    assert np.abs(pts[:, :3]).max() < 2 ** 20
    for k, p in zip(keys[::7], pts[::7]):  # VoxelHashMap: one point in, its key out of downsampling
        m = vc.OracleVhm(orc, 1.0)
        m.add(p[None])
        rows = m.rows()
        assert [int(x) for x in rows["keys"]] == [k] and np.array_equal(rows["points"][0], p)


def test_hot_cloud_sums_are_exact_in_any_order():
    for counts in vc.HOT_COUNTS.values():
        c = vc.hot_cloud(counts)
        rs = np.random.RandomState(3)
        for _ in range(3):
            o = rs.permutation(len(c["voxel"]))
            for v in range(len(counts)):
                rows = o[c["voxel"][o] == v]
                acc = np.zeros(3, np.float32)
                for p in c["pts"][rows, :3]:
                    acc += p  # fp32, one at a time, in this order
                assert np.array_equal(acc.astype(np.float64), c["sum_xyz"][v])


def test_model_rules():
    """the model against itself on the smallest cases: what a `deleted` slot does in each kind of table"""
    k0, k1 = vc.chain(30029, 2, True, vc.NEIGHBOURS)
    for kind in ("vhm", "ogm"):
        t = vc.TableModel(kind, max_age=0, removal_cycle=1)
        t.add_frame([k0])
        t.add_frame([k1])  # k0 is one frame old: removed
        assert t.voxel_num == 1 and [k for _, k, _ in t.slots()] == [k1]
        assert (t.find(k1) is None) == (kind == "vhm")  # cut chain | stepped-over tombstone
        t.add_frame([k1])  # claims the sequence's first slot in either kind; the entry behind it is one frame old: removed
        assert [(s, k, c) for s, k, c in t.slots()] == [(6410, k1, 1)] and t.voxel_num == 1 and t.find(k1) == 6410


# ----------------------------------------------------------------------------------------------------------------- VoxelHashMap
@pytest.mark.parametrize("cap", [30029, 60013])
def test_vhm_probe_limit_one_frame(vhm, cap):
    vc.vhm_probe_limit_one_frame(vhm, cap)


def test_vhm_probe_limit_one_per_frame(vhm):
    vc.vhm_probe_limit_one_per_frame(vhm)


def test_vhm_diverging_chains(vhm):
    vc.vhm_diverging(vhm)


def test_vhm_cut_chain_duplicate_merge(vhm):
    vc.vhm_cut_chain(vhm)


@pytest.mark.parametrize("layout", list(vc.HOT_COUNTS))
def test_vhm_hot_voxels(vhm, layout):
    vc.vhm_hot_voxels(vhm, vc.HOT_COUNTS[layout])


def test_vhm_hot_covariances(vhm):
    print(f"VoxelHashMap, 512 equal covariances per voxel: E_ref = {vc.vhm_hot_covariances(vhm[0]):.3e}")


# ------------------------------------------------------------------------------------------------------------- OccupancyGridMap
def test_ogm_probe_limit_one_frame(ogm):
    vc.ogm_probe_limit_one_frame(ogm)


def test_ogm_probe_limit_one_per_frame(ogm):
    vc.ogm_probe_limit_one_per_frame(ogm)


def test_ogm_diverging_chains(ogm):
    vc.ogm_diverging(ogm)


def test_ogm_tombstones_and_duplicate(ogm):
    vc.ogm_tombstones(ogm)


@pytest.mark.parametrize("layout", list(vc.HOT_COUNTS))
def test_ogm_hot_voxels(ogm, layout):
    (log_odds,) = vc.ogm_hot_voxels(ogm, vc.HOT_COUNTS[layout])
    assert (log_odds == 4.0).all()  # 128 hits and more: clamped


def test_ogm_hot_carving(ogm):
    vc.ogm_hot_carving(ogm)
