"""Engineered probe chains and hot voxels for the two hashed voxel maps (csrc/sp_voxel_table.h): a helper module, no tests, no
fixtures. tests/test_voxel_chains_cpu.py runs every scenario below on the CPU references alone (the oracle's VoxelHashMap, the
restatement of OccupancyGridMap); tests/test_gpu_voxel_hash_map_chains.py and tests/test_gpu_occupancy_grid_chains.py run the same
functions with the device map in the list. Nothing here allows a tolerance: every comparison is ==.

Voxel keys are plain integers (three 21-bit cell fields) and the table's probe sequence is
    slot_id(h, p, cap) = (h + p * ((cap - 2) - h mod (cap - 2))) mod cap,
so keys that share a whole sequence, or only its first slot, can be written down (chain), turned into the points at their cells'
centres (points_of: exact in fp32 at voxel 1.0 and 0.5) and fed to a map under the identity pose. Fed one per frame the slot layout
is the sequential one, which TableModel states a third time in Python integers; fed all in one frame the facts that do not depend
on the order of arrival are still exact.

A map is driven through one small interface. VoxelHashMap (OracleVhm here, the device's adapter in the GPU test): set(name, value),
info(name), add(pts, covs, rgb, intensities), overlap(pts), rows() -> dict of keys / points / covs / rgb / intensities in slot
order. OccupancyGridMap: the interface RestatedMap and DevMap already share."""
import numpy as np

INVALID = (1 << 64) - 1
DELETED = INVALID - 1
LADDER = (30029, 60013, 120011, 240007, 480013, 960017, 1920001, 3840007, 7680017, 15360013, 30720007)
FIELD_BITS, FIELD_OFFSET, FIELD_MASK = 21, 1 << 20, (1 << 21) - 1
PROBES = {"vhm": 100, "ogm": 128}


def stride(h, cap):
    return (cap - 2) - h % (cap - 2)


def slot_id(h, p, cap):
    return (h + p * stride(h, cap)) % cap


def key_of(cell):
    """the key of the cell with these three (signed) indices"""
    x, y, z = (int(c) + FIELD_OFFSET for c in cell)
    assert all(0 <= f <= FIELD_MASK for f in (x, y, z))
    return x | (y << FIELD_BITS) | (z << (2 * FIELD_BITS))


def base_key(cap, first_slot, step, near=key_of((3, 5, 7))):
    """the smallest key >= near whose probe sequence at capacity `cap` starts at first_slot and advances by `step` slots per probe
    (cap and cap - 2 are coprime: the two residues fix the key modulo their product)"""
    m = cap - 2
    assert 0 <= first_slot < cap and 1 <= step <= m
    h = (first_slot * m * pow(m, -1, cap) + (m - step) * cap * pow(cap, -1, m)) % (cap * m)
    h += -((h - near) // (cap * m)) * cap * m
    assert h >= near and slot_id(h, 0, cap) == first_slot and stride(h, cap) == step
    return h


# the chains the scenarios use. 30 029: first slot 20306, then 16939, ...; 60 013: likewise far apart. NEIGHBOURS: a sequence of
# consecutive slots inside one wave's 64 (slots 6410, 6411, 6412: lanes 10, 11, 12), for the scenarios whose rehash moves two entries
# of one key: the two then leave the old table from one wave instruction, in lane order.
BASE = {30029: base_key(30029, 20306, 26662), 60013: base_key(60013, 41234, 33331)}
NEIGHBOURS = base_key(30029, 6410, 1)
NEAR_POINT = np.array([[0.25, 0.25, 0.25, 1.0]], np.float32)  # a harmless voxel next to the origin, on none of the chains


def chain(cap, n, same_stride, base):
    """n valid 63-bit voxel keys, the base first. same_stride: base + j cap (cap - 2), every key shares the base's whole probe
    sequence at capacity cap. Otherwise base + j cap without any key whose h mod (cap - 2) is the base's: one first slot, then apart."""
    if same_stride:
        keys = [base + j * cap * (cap - 2) for j in range(n)]
    else:
        keys, j = [base], 1
        while len(keys) < n:
            if (base + j * cap) % (cap - 2) != base % (cap - 2):
                keys.append(base + j * cap)
            j += 1
    assert all(0 <= k < (1 << 63) for k in keys) and len(set(keys)) == n
    return keys


def cells_of(keys):
    k = np.array(keys, dtype=np.uint64)
    return np.stack([((k >> np.uint64(FIELD_BITS * a)) & np.uint64(FIELD_MASK)).astype(np.int64) - FIELD_OFFSET for a in range(3)], axis=1)


def points_of(keys, voxel, frac=0.5):
    """the fp32 point (x, y, z, 1) at fraction `frac` of each key's cell: ((field - 2^20) + frac) voxel, exact for voxel 1.0 and 0.5"""
    want = (cells_of(keys) + frac) * voxel
    pts = np.ones((len(keys), 4), np.float32)
    pts[:, :3] = want
    assert np.array_equal(pts[:, :3].astype(np.float64), want)
    return pts


class TableModel:
    """The table's rules and the host schedule around them, once more, in Python integers.
    vhm: claim on `invalid` only, 100 probes, removal resets the slot to `invalid` (the chain is cut), the rehash re-inserts in slot
         order and so merges equal keys by adding their counts; an empty cloud is a frame.
    ogm: claim on `invalid` or `deleted`, 128 probes, pruning writes `deleted`, lookups step over `deleted` and stop at `invalid`, the
         rehash claims `invalid` slots only and keeps duplicates; an empty cloud is nothing.
    Per slot: key, count (hit_count), stamp of the last update. No float sums."""

    def __init__(self, kind, rehash_threshold=0.7, max_age=100, removal_cycle=10, removal=True):
        self.kind, self.probes, self.capacity = kind, PROBES[kind], LADDER[0]
        self.rehash_threshold, self.max_age, self.removal_cycle, self.removal = rehash_threshold, max_age, removal_cycle, removal
        self.table, self.voxel_num, self.frame = {}, 0, 0  # slot -> [key, count, stamp]

    def key_at(self, s):
        return self.table[s][0] if s in self.table else INVALID

    def insert(self, key, count, stamp):
        for p in range(self.probes):
            s = slot_id(key, p, self.capacity)
            seen = self.key_at(s)
            if seen == INVALID or (self.kind == "ogm" and seen == DELETED):
                self.table[s] = [key, 0, stamp]
                self.voxel_num += 1
            elif seen != key:
                continue
            self.table[s][1] += count
            self.table[s][2] = stamp
            return s
        return None  # dropped

    def find(self, key):
        for p in range(self.probes):
            s = slot_id(key, p, self.capacity)
            if self.key_at(s) == key:
                return s
            if self.key_at(s) == INVALID:
                return None
        return None

    def count(self, key):
        """what a lookup of the key sees: the count of the first entry on its sequence, 0 for none"""
        s = self.find(key)
        return 0 if s is None else self.table[s][1]

    def slots(self):
        return [(s, e[0], e[1]) for s, e in sorted(self.table.items()) if e[0] != DELETED]

    def rehash(self):
        old, self.table, self.voxel_num = self.slots_with_stamps(), {}, 0
        self.capacity = next(c for c in LADDER if c > self.capacity)
        for key, count, stamp in old:
            if self.kind == "vhm":
                self.insert(key, count, stamp)
                continue
            for p in range(self.probes):
                s = slot_id(key, p, self.capacity)
                if s not in self.table:
                    self.table[s] = [key, count, stamp]
                    self.voxel_num += 1
                    break

    def slots_with_stamps(self):
        return [tuple(e) for _, e in sorted(self.table.items()) if e[0] != DELETED]

    def add_frame(self, keys):
        if self.kind == "ogm" and not keys:
            return
        if self.rehash_threshold < self.voxel_num / self.capacity:
            self.rehash()
        for k in keys:
            self.insert(k, 1, self.frame)
        if self.kind == "vhm" and self.removal and self.frame % self.removal_cycle == 0 and self.frame > self.max_age:
            self.table = {s: e for s, e in self.table.items() if e[2] >= self.frame - self.max_age}
            self.voxel_num = len(self.table)
        if self.kind == "ogm" and self.removal and self.frame >= self.max_age:
            for e in self.table.values():
                if e[0] != DELETED and self.frame - e[2] > self.max_age:
                    e[:] = [DELETED, 0, 0]
            self.voxel_num = len(self.slots())
        self.frame += 1


def f32_ratio(a, b):
    return float(np.float32(a) / np.float32(b))


# ------------------------------------------------------------------------------------------------------------- VoxelHashMap
class OracleVhm:
    """oracle.voxel_hash_map behind the interface the scenarios drive"""

    def __init__(self, orc, voxel):
        self.m = orc.voxel_hash_map(voxel)

    def set(self, name, value):
        self.m.set(name, value)

    def info(self, name):
        return self.m.info(name)

    def add(self, pts, covs=None, rgb=None, intensities=None):
        self.m.add_point_cloud(np.asarray(pts, np.float32).reshape(-1, 4), None, covs=covs, rgb=rgb, intensities=intensities)

    def overlap(self, pts):
        return self.m.overlap_ratio(pts)

    def rows(self):
        return self.m.downsampling((0.0, 0.0, 0.0), 1e7)


EMPTY = np.zeros((0, 4), np.float32)


def vhm_agrees(m, model, min_num_point=1, lookups=()):
    """one map against the model: voxel_num, capacity, the exported keys (slot order) and their centroids, one lookup per key"""
    assert m.info("voxel_num") == model.voxel_num and m.info("capacity") == model.capacity
    want = [k for _, k, c in model.slots() if c >= min_num_point]
    rows = m.rows()
    assert [int(k) for k in rows["keys"]] == want
    assert np.array_equal(rows["points"], points_of(want, 1.0))  # every point sits at its cell's centre: the mean is that point
    for k in lookups:
        assert m.overlap(points_of([k], 1.0)) == (1.0 if model.count(k) >= max(min_num_point, 1) else 0.0), hex(k)


def vhm_seed_second_capacity(m, model):
    """30 029 -> 60 013 slots with one voxel in the table: threshold 0, one point, an empty frame that rehashes, threshold back"""
    m.set("rehash_threshold", 0.0)
    model.rehash_threshold = 0.0
    m.add(NEAR_POINT)
    model.add_frame([key_of((0, 0, 0))])
    assert m.info("capacity") == model.capacity == 30029
    m.add(EMPTY)
    model.add_frame([])
    assert m.info("capacity") == model.capacity == 60013 and m.info("voxel_num") == model.voxel_num == 1
    m.set("rehash_threshold", 0.7)
    model.rehash_threshold = 0.7


def vhm_probe_limit_one_frame(maps, cap):
    """150 keys on one probe sequence in one add_point_cloud: 100 slots, 100 voxels, whichever 100 arrive first."""
    keys = chain(cap, 150, True, BASE[cap])
    pts = points_of(keys, 1.0)
    for m in maps:
        model = TableModel("vhm", removal=False)
        m.set("remove_old_data_cycle", 0)
        extra = []
        if cap != LADDER[0]:
            vhm_seed_second_capacity(m, model)
            extra = [key_of((0, 0, 0))]
        m.add(pts)
        model.add_frame(keys)
        assert model.voxel_num == 100 + len(extra)
        assert m.info("voxel_num") == model.voxel_num and m.info("capacity") == model.capacity == cap
        rows = m.rows()
        got = [int(k) for k in rows["keys"] if int(k) not in extra]
        assert len(rows["keys"]) == 100 + len(extra) and len(got) == 100 == len(set(got)) and set(got) <= set(keys)
        by_key = {int(k): p for k, p in zip(rows["keys"], rows["points"])}
        assert all(np.array_equal(by_key[k], points_of([k], 1.0)[0]) for k in got)
        ratio = m.overlap(pts)
        assert ratio == f32_ratio(100, 150) == 0.6666666865348816, ratio


def vhm_probe_limit_one_per_frame(maps):
    """The same 150 keys, one per call: the first 100 get in, in the model's slots; with 99, 100 and 101 keys fed the map holds 99,
    100 and 100 voxels (checked on the way)."""
    keys = chain(30029, 150, True, BASE[30029])
    pts = points_of(keys, 1.0)
    for m in maps:
        model = TableModel("vhm", removal=False)
        m.set("remove_old_data_cycle", 0)
        for i, k in enumerate(keys):
            m.add(pts[i:i + 1])
            model.add_frame([k])
            assert m.info("voxel_num") == model.voxel_num == min(i + 1, 100), i
            if i + 1 in (99, 100, 101):
                vhm_agrees(m, model)
        vhm_agrees(m, model)
        assert {k for _, k, _ in model.slots()} == set(keys[:100])
        assert m.overlap(pts[:100]) == 1.0 and m.overlap(pts[100:]) == 0.0


def vhm_diverging(maps):
    """64 keys that share their first slot and nothing else, in one frame (one wave, every lane's first swap on one slot): all 64
    get in, each on its own second slot or the shared first."""
    keys = chain(30029, 64, False, BASE[30029])
    pts = points_of(keys, 1.0)
    for m in maps:
        model = TableModel("vhm", removal=False)
        m.set("remove_old_data_cycle", 0)
        m.add(pts)
        model.add_frame(keys)
        assert m.info("voxel_num") == model.voxel_num == 64 and m.overlap(pts) == 1.0
        rows = m.rows()
        assert sorted(int(k) for k in rows["keys"]) == sorted(keys)
        assert {s for s, _, _ in model.slots()} == {slot_id(keys[0], 0, 30029)} | {slot_id(k, 1, 30029) for k in keys[1:]}
        by_key = {int(k): p for k, p in zip(rows["keys"], rows["points"])}
        assert all(np.array_equal(by_key[k], points_of([k], 1.0)[0]) for k in keys)


def vhm_cut_chain(maps):
    """K0, K1, K2 on one sequence, max_staleness 2, removal every frame. Frames K0, K1, K2, K2: K0 goes stale and its slot, the
    sequence's first, is reset to `invalid`; K1 and K2 sit behind the cut where no lookup reaches them. Frame K2: the insert claims
    the cut slot, the table holds K2 twice (1 point in front, 2 behind) and K1 goes stale. A rehash merges the two: 3 points."""
    k0, k1, k2 = keys = chain(30029, 3, True, NEIGHBOURS)
    p = [points_of([k], 1.0) for k in keys]
    for m in maps:
        model = TableModel("vhm", max_age=2, removal_cycle=1)
        m.set("max_staleness", 2)
        m.set("remove_old_data_cycle", 1)
        for i in (0, 1, 2, 2):
            m.add(p[i])
            model.add_frame([keys[i]])
        assert model.voxel_num == 2 and [k for _, k, _ in model.slots()] == [k1, k2] and model.find(k1) is None
        vhm_agrees(m, model, lookups=keys)
        assert m.overlap(p[1]) == 0.0 and m.overlap(p[2]) == 0.0  # behind the cut
        m.add(p[2])
        model.add_frame([k2])
        assert model.voxel_num == 2 and [(k, c) for _, k, c in model.slots()] == [(k2, 1), (k2, 2)]
        vhm_agrees(m, model, lookups=keys)
        assert m.overlap(p[2]) == 1.0
        m.set("min_num_point", 2)
        vhm_agrees(m, model, min_num_point=2, lookups=keys)
        assert m.overlap(p[2]) == 0.0 and len(m.rows()["keys"]) == 1  # the lookup meets the one-point entry first
        m.set("min_num_point", 1)
        m.set("rehash_threshold", 0.0)
        model.rehash_threshold = 0.0
        m.add(EMPTY)
        model.add_frame([])
        assert model.capacity == 60013 and [(k, c) for _, k, c in model.slots()] == [(k2, 3)]
        vhm_agrees(m, model, lookups=keys)
        for thr, ratio in ((3, 1.0), (4, 0.0)):  # the merged count is exactly 3
            m.set("min_num_point", thr)
            assert m.overlap(p[2]) == ratio
            vhm_agrees(m, model, min_num_point=thr)


def hot_cloud(counts, seed=11):
    """sum(counts) <= 8192 points in len(counts) <= 7 voxels, shuffled. Coordinates are cell + j / 256 with cells 1 .. 7 and
    j < 128 (one voxel at size 1.0 and at 0.5), colours multiples of 1 / 256 in [0, 1], intensities integers 0 .. 255: every partial
    sum of at most 8192 such values is a multiple of 2^-8 below 2^16, 24 bits, exact in fp32 in ANY order. The counts are powers of
    two, so 1 / count and the mean are exact too. More than 8192 points would break that."""
    assert sum(counts) <= 8192 and len(counts) <= 7 and all(c & (c - 1) == 0 for c in counts)
    rs = np.random.RandomState(seed)
    cells = np.array([(c, 8 - c, (3 * c) % 7 + 1) for c in range(1, len(counts) + 1)])
    voxel = rs.permutation(np.repeat(np.arange(len(counts)), counts))
    n = len(voxel)
    xyz = cells[voxel] + rs.randint(0, 128, (n, 3)) / 256.0
    rgb = rs.randint(0, 257, (n, 4)) / 256.0
    rgb[:, 3] = 1.0
    inten = rs.randint(0, 256, n).astype(np.float64)
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = xyz
    out = dict(pts=pts, rgb=rgb.astype(np.float32), intensities=inten.astype(np.float32), voxel=voxel, cells=cells, counts=counts)
    for name, a in (("sum_xyz", xyz), ("sum_rgb", rgb), ("sum_intensity", inten)):  # float64 sums per voxel
        out[name] = np.stack([a[voxel == v].sum(axis=0) for v in range(len(counts))])
        assert np.array_equal(out[name].astype(np.float32).astype(np.float64), out[name])
    return out


HOT_COUNTS = {"one voxel": (8192,), "seven voxels": (4096, 2048, 1024, 512, 256, 128, 128)}


def vhm_hot_voxels(maps, counts):
    """8192 points of one frame in one voxel, or in seven: counts exact (through min_num_point), centroid, colour and intensity
    bit-equal to the float64 mean. A lost or doubled atomic add changes a count or a sum."""
    c = hot_cloud(counts)
    cnt = np.array(counts, np.float64)
    keys = [key_of(cell) for cell in c["cells"]]
    order = np.argsort(np.array(keys, dtype=np.uint64))
    q = points_of(keys, 1.0, 0.25)
    for m in maps:
        m.set("remove_old_data_cycle", 0)
        m.add(c["pts"], rgb=c["rgb"], intensities=c["intensities"])
        assert m.info("voxel_num") == len(counts) and m.info("capacity") == 30029
        rows = m.rows()
        o = np.argsort(rows["keys"])
        assert [int(k) for k in rows["keys"][o]] == [keys[i] for i in order] and rows["covs"] is None
        assert np.array_equal(rows["points"][o][:, :3], (c["sum_xyz"] / cnt[:, None])[order].astype(np.float32))
        assert (rows["points"][:, 3] == 1.0).all()
        assert np.array_equal(rows["rgb"][o], (c["sum_rgb"] / cnt[:, None])[order].astype(np.float32))
        assert np.array_equal(rows["intensities"][o], (c["sum_intensity"] / cnt)[order].astype(np.float32))
        for thr in sorted({t for n in counts for t in (n, n + 1)}):
            m.set("min_num_point", thr)
            assert m.overlap(q) == f32_ratio(sum(n >= thr for n in counts), len(counts)), thr
            assert len(m.rows()["keys"]) == sum(n >= thr for n in counts)


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def vhm_hot_covariances(m):
    """512 points in each of seven voxels, every point of a voxel with the same well-conditioned covariance (eigenvalues 0.01, 0.04,
    0.25, rotated, another rotation per voxel). The log-Euclidean mean of equal matrices is that matrix: the expected output is the
    fp32 input itself, read as float64. Returns the largest relative error of the map's output, max |got - want| / max |want|."""
    c = hot_cloud((512,) * 7)
    want = []
    for v in range(7):
        Rm = rotation(0.3 + 0.4 * v, -0.2 + 0.3 * v, 0.7 - 0.5 * v)
        C = Rm @ np.diag([0.01, 0.04, 0.25]) @ Rm.T
        want.append(((C + C.T) / 2).astype(np.float32))
    covs = np.zeros((len(c["voxel"]), 4, 4), np.float32)
    covs[:, :3, :3] = np.stack(want)[c["voxel"]]
    keys = [key_of(cell) for cell in c["cells"]]
    m.set("remove_old_data_cycle", 0)
    m.add(c["pts"], covs=covs.reshape(-1, 16))
    rows = m.rows()
    assert sorted(int(k) for k in rows["keys"]) == sorted(keys) and m.info("voxel_num") == 7
    got = rows["covs"].reshape(-1, 4, 4).transpose(0, 2, 1)
    assert not got[:, 3, :].any() and not got[:, :, 3].any()
    err = 0.0
    for k, g in zip(rows["keys"], got):
        w = want[keys.index(int(k))].astype(np.float64)
        err = max(err, np.abs(g[:3, :3] - w).max() / np.abs(w).max())
    for thr, ratio in ((512, 1.0), (513, 0.0)):
        m.set("min_num_point", thr)
        assert m.overlap(points_of(keys, 1.0, 0.25)) == ratio
    return err


# ---------------------------------------------------------------------------------------------------------- OccupancyGridMap
OGM_VOXEL = 0.5
ONE_HIT = 0.7005671858787537  # 1 / (1 + exp(-0.85)) in fp32: the probability of a voxel hit once, default log-odds


def sorted_pairs(exp):
    return sorted(zip((int(k) for k in exp["keys"]), (int(h) for h in exp["hit_count"])))


def ogm_agrees(m, model):
    """one map against the model: voxel_num, capacity, the export's keys and hit counts in slot order"""
    assert m.info("voxel_num") == model.voxel_num and m.info("capacity") == model.capacity
    e = m.export()
    assert [(int(k), int(h)) for k, h in zip(e["keys"], e["hit_count"])] == [(k, c) for _, k, c in model.slots()]
    return e


def ogm_chain_settings(m, pruning):
    m.set("free_space_updates_enabled", 0)  # a carved ray to a chain point would walk millions of cells
    m.set("voxel_pruning_enabled", pruning)


def ogm_probe_limit_one_frame(maps):
    """130 keys on one probe sequence in one frame: 128 slots, 128 voxels, whichever 128 arrive first."""
    keys = chain(30029, 130, True, BASE[30029])
    pts = points_of(keys, OGM_VOXEL)
    for m in maps:
        ogm_chain_settings(m, 0)
        m.add_point_cloud(pts)
        e = m.export()
        got = [int(k) for k in e["keys"]]
        assert m.info("voxel_num") == 128 == len(got) == len(set(got)) and set(got) <= set(keys)
        assert (e["hit_count"] == 1).all() and (e["miss_count"] == 0).all()
        ratio = m.compute_overlap_ratio(pts)
        assert ratio == f32_ratio(128, 130) == 0.9846153855323792, ratio


def ogm_probe_limit_one_per_frame(maps):
    """129 keys of one sequence, one per frame: 127, 128 and 129 keys fed leave 127, 128 and 128 voxels, in the model's slots."""
    keys = chain(30029, 129, True, BASE[30029])
    pts = points_of(keys, OGM_VOXEL)
    for m in maps:
        model = TableModel("ogm", removal=False)
        ogm_chain_settings(m, 0)
        for i, k in enumerate(keys):
            m.add_point_cloud(pts[i:i + 1])
            model.add_frame([k])
            assert m.info("voxel_num") == model.voxel_num == min(i + 1, 128), i
            if i + 1 in (127, 128, 129):
                e = ogm_agrees(m, model)
                assert (e["hit_count"] == 1).all() and len(e["keys"]) == min(i + 1, 128)
        assert m.compute_overlap_ratio(pts[:128]) == 1.0 and m.compute_overlap_ratio(pts[128:]) == 0.0
        assert m.voxel_probability(pts[127, :3]) == ONE_HIT and m.voxel_probability(pts[128, :3]) == 0.5


def ogm_diverging(maps):
    """64 keys that share their first slot and nothing else, in one frame: all 64 get in."""
    keys = chain(30029, 64, False, BASE[30029])
    pts = points_of(keys, OGM_VOXEL)
    for m in maps:
        model = TableModel("ogm", removal=False)
        ogm_chain_settings(m, 0)
        m.add_point_cloud(pts)
        model.add_frame(keys)
        assert m.info("voxel_num") == model.voxel_num == 64 and m.compute_overlap_ratio(pts) == 1.0
        assert sorted_pairs(m.export()) == sorted((k, 1) for k in keys)


def ogm_tombstones(maps):
    """K0, K1, K2 on one sequence, stale_frame_threshold 2, frames K0, K1, K2, K2, K2. After the fourth K0 is pruned: its slot, the
    sequence's first, holds `deleted` and every lookup of K1 and K2 has to step over it. The fifth frame's hit claims that `deleted`
    slot before it reaches K2's own: the table holds K2 twice, one hit in front and two behind, and a lookup answers with the one in
    front. A rehash keeps both. Returns what each map answered, for the caller to compare the maps with one another."""
    k0, k1, k2 = keys = chain(30029, 3, True, NEIGHBOURS)
    p = [points_of([k], OGM_VOXEL) for k in keys]
    answers = []
    for m in maps:
        model = TableModel("ogm", max_age=2)
        ogm_chain_settings(m, 1)
        m.set("stale_frame_threshold", 2)
        for i in (0, 1, 2, 2):
            m.add_point_cloud(p[i])
            model.add_frame([keys[i]])
        assert [(k, c) for _, k, c in model.slots()] == [(k1, 1), (k2, 2)] and model.voxel_num == 2
        assert model.key_at(slot_id(k0, 0, 30029)) == DELETED and (model.count(k1), model.count(k2)) == (1, 2)
        ogm_agrees(m, model)
        got = [m.voxel_probability(p[0][0, :3]), m.voxel_probability(p[1][0, :3]), m.voxel_probability(p[2][0, :3]),
               m.compute_overlap_ratio(np.concatenate(p))]
        assert got[0] == 0.5 and got[1] == ONE_HIT and got[2] > ONE_HIT and got[3] == f32_ratio(2, 3)
        m.add_point_cloud(p[2])
        model.add_frame([k2])
        assert [(k, c) for _, k, c in model.slots()] == [(k2, 1), (k2, 2)] and model.voxel_num == 2 and model.count(k2) == 1
        assert model.key_at(slot_id(k2, 0, 30029)) == k2 and model.key_at(slot_id(k2, 1, 30029)) == DELETED
        e = ogm_agrees(m, model)
        assert e["last_updated"].tolist() == [4, 3]
        got += [m.voxel_probability(p[1][0, :3]), m.voxel_probability(p[2][0, :3]), m.compute_overlap_ratio(np.concatenate(p))]
        assert got[4] == 0.5 and got[5] == ONE_HIT and got[6] == f32_ratio(1, 3)
        m.set("rehash_threshold", 0.0)
        m.set("voxel_pruning_enabled", 0)
        model.rehash_threshold, model.removal = 0.0, False
        m.add_point_cloud(NEAR_POINT)
        model.add_frame([key_of((0, 0, 0))])
        assert model.capacity == 60013 and model.voxel_num == 3
        assert sorted((k, c) for _, k, c in model.slots()) == [(key_of((0, 0, 0)), 1), (k2, 1), (k2, 2)]
        assert m.info("voxel_num") == 3 and m.info("capacity") == 60013
        e = m.export()
        assert sorted_pairs(e) == sorted((k, c) for _, k, c in model.slots())
        # whichever entry sits on the first slot of K2's sequence in the new table answers the lookup ...
        front, behind = slot_id(k2, 0, 60013), slot_id(k2, 1, 60013)
        assert sorted(s for s, k, _ in model.slots() if k == k2) == sorted((front, behind))
        hits = [int(h) for k, h in zip(e["keys"], e["hit_count"]) if int(k) == k2]  # slot order
        in_front = hits[0] if front < behind else hits[1]
        got.append(m.voxel_probability(p[2][0, :3]))
        assert (got[-1] == ONE_HIT) == (in_front == 1) and (got[-1] > ONE_HIT) == (in_front == 2)
        # ... and that is the one the model puts there: the old table's slots re-enter in slot order
        assert in_front == model.count(k2) == 1
        ogm_agrees(m, model)
        answers.append(got)
    return answers


def ogm_hot_voxels(maps, counts):
    """The dyadic cloud of hot_cloud at voxel 0.5, carving off: hit_count exact, the three sums of export() bit-equal to the float64
    sums. Returns each map's log-odds by key, for the caller to compare the maps with one another."""
    c = hot_cloud(counts)
    keys = np.array([key_of(2 * cell) for cell in c["cells"]], dtype=np.uint64)
    order = np.argsort(keys)
    log_odds = []
    for m in maps:
        m.set("free_space_updates_enabled", 0)
        m.add_point_cloud(c["pts"], None, None, c["rgb"], c["intensities"])
        assert m.info("voxel_num") == len(counts)
        e = m.export()
        o = np.argsort(e["keys"])
        assert np.array_equal(e["keys"][o], keys[order])
        assert np.array_equal(e["hit_count"][o], np.array(counts)[order]) and (e["miss_count"] == 0).all()
        assert np.array_equal(e["sum_xyz"][o].astype(np.float64), c["sum_xyz"][order])
        assert np.array_equal(e["rgb_sums"][o].astype(np.float64), c["sum_rgb"][order])
        assert np.array_equal(e["intensity_sums"][o].astype(np.float64), c["sum_intensity"][order])
        log_odds.append(e["log_odds"][o])
    return log_odds


def ogm_hot_carving(maps):
    """Carving on, the sensor at the centre of cell (0, 0, 0), 4096 points in the one voxel that is the sixth cell along +x, the
    sensor's own counted: every ray posts its misses to the same five cells in front of it. miss_count 4096 on each of the five,
    hit_count 4096 on the sixth, six voxels, log-odds clamped at both ends. Returns each map's export by key."""
    rs = np.random.RandomState(5)
    pts = np.ones((4096, 4), np.float32)
    pts[:, :3] = np.array([2.5, 0.0, 0.0]) + rs.randint(0, 128, (4096, 3)) / 256.0  # map frame: cell (5, 0, 0)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = 0.25
    pts[:, :3] -= 0.25  # sensor frame; the sum back is exact
    keys = [key_of((x, 0, 0)) for x in range(6)]
    exports = []
    for m in maps:
        m.add_point_cloud(pts, pose)
        # the visit estimate is 4096 x 6 cells, above 0.7 x 30 029: the table grows one step before the walk
        assert m.info("voxel_num") == 6 and m.info("capacity") == 60013
        e = m.export()
        o = np.argsort(e["keys"])
        assert [int(k) for k in e["keys"][o]] == keys
        assert e["miss_count"][o].tolist() == [4096] * 5 + [0] and e["hit_count"][o].tolist() == [0] * 5 + [4096]
        assert e["log_odds"][o].tolist() == [-4.0] * 5 + [4.0]
        exports.append({k: v[o] for k, v in e.items()})
    return exports
