"""The pieces the search structures share (csrc/sp_spatial.h) on their own, through sp_internal_bbox, sp_internal_morton_keys and
sp_internal_sorted_insert (csrc/spatial_probes.hip): a bounding box or a Morton key that is wrong inside the BVH cannot be seen
from outside (its search is exact, a bad curve only makes it slower), and a box that is too small gives brute force rare wrong
lists. Every comparison is exact equality against NumPy / Python integers."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028234663852886e38)
SENTINEL = np.array([0xFFFFFFFF] * 3 + [0] * 3, dtype=np.uint32)


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------ bounding box

def decode(words):
    """Inverse of the order-preserving float -> u32 map: sign bit set <=> the float was >= +0."""
    w = np.asarray(words, dtype=np.uint32)
    bits = np.where(w & np.uint32(0x80000000), w & np.uint32(0x7FFFFFFF), ~w)
    return bits.astype(np.uint32).view(np.float32)


def bbox_words(sp, pts, workgroups):
    out = torch.full((6,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d = dev(pts) if len(pts) else None
    sp.check(sp._lib.lib().sp_internal_bbox(sp._ptr(d), len(pts), workgroups, sp._ptr(out), sp._stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def check_box(sp, pts, workgroups):
    got = bbox_words(sp, pts, workgroups)
    ok = np.isfinite(pts[:, :3]).all(axis=1)
    if not ok.any():
        assert np.array_equal(got, SENTINEL)
        return
    want = np.concatenate([pts[ok, :3].min(axis=0), pts[ok, :3].max(axis=0)])
    assert (decode(got) == want).all(), (decode(got), want)  # (==: the sign of a zero is not pinned)


def clouds(n, workgroups):
    rng = np.random.default_rng(1000 * n + workgroups)
    base = np.zeros((n, 4), dtype=np.float32)
    base[:, :3] = (rng.standard_normal((n, 3)) * 100.0).astype(np.float32)
    base[:, 3] = 1.0
    finite = base.copy()  # negative values on every axis, and both zeros
    finite[rng.integers(0, n), 0] = 0.0
    finite[rng.integers(0, n), 1] = -0.0
    yield "finite", finite
    holes = base.copy()  # about 10 % of the rows lose one coordinate
    bad = np.flatnonzero(rng.random(n) < 0.1)
    holes[bad, rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), len(bad))
    yield "holes", holes
    # the extremes where a tail bug would lose them: index 0, n - 1, and the last slot below n of a lane whose group of four
    # loads (i, i + stride, i + 2 stride, i + 3 stride) is partly past n — the first lane, the last lane, and the first lane
    # that is one slot short; unless n is a multiple of 4 stride at least one of the three groups is partly filled
    ext = base.copy()
    stride = workgroups * 256
    last_slot = lambda lane: lane + (n - 1 - lane) // stride * stride if lane < n else n // 2  # noqa: E731
    ext[n // 2, 2] = -3e6
    ext[last_slot(stride - 1), 2] = 3e6
    ext[last_slot(0), 1] = -2e6
    ext[last_slot(n % stride), 1] = 2e6
    ext[0, 0] = -1e6
    ext[n - 1, 0] = 1e6
    yield "extremes", ext
    none = base.copy()
    none[:, rng.integers(0, 3)] = np.nan
    none[::2, 0] = np.inf
    yield "none finite", none
    if n >= 2:  # a single finite row, the last one
        one = none.copy()
        one[n - 1, :3] = (-1.5, 0.0, 2.5)
        yield "one finite", one


@pytest.mark.parametrize("workgroups", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 5000])
def test_bbox_matches_numpy(sp, n, workgroups):
    for _, pts in clouds(n, workgroups):
        check_box(sp, pts, workgroups)


def test_bbox_of_nothing_is_the_sentinel(sp):
    assert np.array_equal(bbox_words(sp, np.zeros((0, 4), dtype=np.float32), 1), SENTINEL)


# ------------------------------------------------------------------------------------------------------------ Morton keys

CELLS = {0: (65535, 65534), 1: (2097152, 2097151)}  # mode: scale, clamp (0: the BVH's, 1: the octree's)


def interleave3(c):
    key = 0
    for b in range(21):
        for a in range(3):
            key |= ((c[a] >> b) & 1) << (3 * b + a)
    return key


def expected_keys(quarters, lo_q, ext_q, mode):
    """quarters: int coordinates in units of 1/4. (v - lo) / ext * scale is exact in binary32 for these inputs (a difference of
    <= 10 bits, a division by a power of two, a product below 2^24 inside the box; outside it the clamp decides whatever the
    rounding), so the cell is floor(j * scale / ext_q) in integers."""
    scale, cmax = CELLS[mode]
    keys = []
    for row in quarters:
        c = [0 if ext_q[a] == 0 else min(max((row[a] - lo_q[a]) * scale // ext_q[a], 0), cmax) for a in range(3)]
        keys.append(interleave3(c))
    return np.array(keys, dtype=np.uint64)


@pytest.fixture(scope="module")
def key_points():
    rng = np.random.default_rng(7)
    q = rng.integers(-128, 129, (900, 3))                       # inside [-32, 32]^3, faces included by chance ...
    q[:40] = rng.choice([-128, 128], (40, 3))                   # ... and on purpose: corners and both faces of every axis
    q[40:80, 0] = rng.choice([-128, 128], 40)
    out = rng.integers(-400, 401, (80, 3))                      # outside: clamped
    q = np.concatenate([q, out, q[:50]])                        # duplicates
    pts = np.ones((len(q), 4), dtype=np.float32)
    pts[:, :3] = q.astype(np.float32) * np.float32(0.25)
    bad = rng.choice(len(q), 30, replace=False)
    pts[bad, rng.integers(0, 3, 30)] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), 30)
    return q, pts


@pytest.mark.parametrize("flat_axis", [None, 2])
@pytest.mark.parametrize("mode", [0, 1])
def test_morton_keys_match_integer_arithmetic(sp, key_points, mode, flat_axis):
    q, pts = key_points
    lo_q, ext_q = [-128, -128, -128], [256, 256, 256]
    if flat_axis is not None:
        ext_q[flat_axis] = 0
    lo = np.array(lo_q, dtype=np.float32) * np.float32(0.25)
    hi = lo + np.array(ext_q, dtype=np.float32) * np.float32(0.25)
    keys = torch.zeros(len(pts), dtype=torch.int64, device="cuda")
    d_pts, d_lo, d_hi = dev(pts), dev(lo), dev(hi)
    sp.check(sp._lib.lib().sp_internal_morton_keys(sp._ptr(d_pts), len(pts), sp._ptr(d_lo), sp._ptr(d_hi), mode, sp._ptr(keys),
                                                   sp._stream()))
    torch.cuda.synchronize()
    got = keys.cpu().numpy().view(np.uint64)
    want = expected_keys(q.tolist(), lo_q, ext_q, mode)
    want[~np.isfinite(pts[:, :3]).all(axis=1)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    assert np.array_equal(got, want)
    assert len(np.unique(want)) > 500  # the cases are not all one key


# ------------------------------------------------------------------------------------------------------------ sorted insertion

ROWS, M = 256, 64


@pytest.fixture(scope="module")
def candidates():
    """256 rows of 64 candidates: eight distinct distances (ties everywhere), about one in ten replaced by NaN, +inf or FLT_MAX,
    the indices a permutation per row — and per order every row's full expected list, to be cut at k."""
    rng = np.random.default_rng(11)
    values = np.array([0.0, 0.25, 1.0, 1.5, 2.0, 3.0, 7.5, 1e30], dtype=np.float32)
    d = values[rng.integers(0, 8, (ROWS, M))]
    special = rng.random((ROWS, M)) < 0.1
    d[special] = rng.choice(np.array([np.nan, np.inf, FLT_MAX], dtype=np.float32), int(special.sum()))
    d[0, :] = np.nan  # a row that takes nothing
    d[1, :] = 2.0     # a row of one distance
    idx = np.stack([rng.permutation(M) for _ in range(ROWS)]).astype(np.int32)
    full = {0: [], 1: []}
    for r in range(ROWS):
        taken = [j for j in range(M) if d[r, j] < FLT_MAX]  # NaN compares false; +inf and FLT_MAX never beat an empty slot
        full[0].append(sorted(taken, key=lambda j: d[r, j]))  # Python's sort is stable: the first arrival stays first
        full[1].append(sorted(taken, key=lambda j: (d[r, j], idx[r, j])))
    return d, idx, full


@pytest.mark.parametrize("order,kcap,k", [(0, 1, 1), (0, 10, 1), (0, 10, 7), (0, 10, 10), (0, 100, 100),
                                          (1, 1, 1), (1, 10, 1), (1, 10, 7), (1, 10, 10), (1, 32, 32)])
def test_sorted_insert_matches_a_sort(sp, candidates, order, kcap, k):
    d, idx, full = candidates
    want_d = np.full((ROWS, k), FLT_MAX, dtype=np.float32)
    want_i = np.full((ROWS, k), -1, dtype=np.int32)
    for r in range(ROWS):
        js = full[order][r][:k]
        want_d[r, :len(js)] = d[r, js]
        want_i[r, :len(js)] = idx[r, js]
    d_dev, i_dev = dev(d), dev(idx)
    d_out = torch.full((ROWS, k), -1.0, dtype=torch.float32, device="cuda")
    i_out = torch.full((ROWS, k), -7, dtype=torch.int32, device="cuda")
    sp.check(sp._lib.lib().sp_internal_sorted_insert(order, kcap, k, sp._ptr(d_dev), sp._ptr(i_dev), ROWS, M, sp._ptr(d_out),
                                                     sp._ptr(i_out), sp._stream()))
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want_d)
    assert np.array_equal(i_out.cpu().numpy(), want_i)
