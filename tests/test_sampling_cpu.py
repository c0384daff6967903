"""Weighted and mixed random sampling without a device: the C ABI's exports and argument checks (SP_ERR_INVALID_ARGUMENT before
any HIP call), the CPU restatement of the two reference operators (tests/cpp/sampling_restate.cpp; filter/preprocess_operator/
weighted_sampling_operator.hpp:29-95, mixed_random_sampling_operator.hpp:28-105) on the reference's own known answers
(cpp/tests/test_preprocess_filter.cpp:202-540), and the tie rule the device implements (include/sycl_points_amd.h,
sp_weighted_sample_flags) against the restatement's literal heap: by hand, and over every arrangement of 8 keys from 3 values.
The GPU suite (tests/test_gpu_sampling.py) holds the device to this restatement, flags bit for bit; its cases and helpers live
here so that the margins its random cases rely on are checked without a device too."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = np.float32(np.nan)
TILE = 1024  # points per workgroup of the sampling kernels (csrc/sampling.hip, kSampTile)


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libsampling_restate.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "sampling_restate.cpp"), "-o", so])
    R = C.CDLL(so)
    vp, u64, u32, f = C.c_void_p, C.c_uint64, C.c_uint32, C.c_float
    R.sampling_weighted_restate.restype = C.c_int
    R.sampling_weighted_restate.argtypes = [u32, vp, u64, u64, vp]
    R.sampling_mixed_restate.restype = C.c_int
    R.sampling_mixed_restate.argtypes = [u32, vp, u64, u64, f, vp]
    R.sampling_draws.restype = None
    R.sampling_draws.argtypes = [u32, u64, vp]
    R.sampling_keys.restype = None
    R.sampling_keys.argtypes = [vp, vp, u64, vp]
    R.sampling_heap_select.restype = None
    R.sampling_heap_select.argtypes = [vp, u64, u64, vp]
    R.sampling_uniform_positions.restype = None
    R.sampling_uniform_positions.argtypes = [u32, u64, u64, u64, vp]
    return R


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return build_restatement(tmp_path_factory.mktemp("sampling"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def weighted_restate(R, seed, w, m):
    w = np.ascontiguousarray(w, np.float32)
    flags = np.full(len(w), 7, np.uint8)
    return R.sampling_weighted_restate(seed, _p(w), len(w), m, _p(flags)), flags


def mixed_restate(R, seed, w, m, ratio):
    w = np.ascontiguousarray(w, np.float32)
    flags = np.full(len(w), 7, np.uint8)
    return R.sampling_mixed_restate(seed, _p(w), len(w), m, ratio, _p(flags)), flags


def draws(R, seed, count):
    u = np.empty(count, np.float32)
    R.sampling_draws(seed, count, _p(u))
    return u


def keys_of(R, w, u):
    w, u = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(u, np.float32)
    assert len(u) >= int((w > 0).sum())
    k = np.empty(len(w), np.float32)
    R.sampling_keys(_p(w), _p(u), len(w), _p(k))
    return k


def heap_select(R, keys, m):
    keys = np.ascontiguousarray(keys, np.float32)
    flags = np.empty(len(keys), np.uint8)
    R.sampling_heap_select(_p(keys), len(keys), m, _p(flags))
    return flags


def uniform_positions(R, seed, weighted_draws, Rn, U):
    pos = np.empty(U, np.uint64)
    R.sampling_uniform_positions(seed, weighted_draws, Rn, U, _p(pos))
    return pos


def ordered(keys):
    """float32 -> int64 that orders as the floats do, adjacent floats one apart (-0 and +0 coincide)."""
    b = np.ascontiguousarray(keys, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def threshold_gap_ulp(keys, m):
    """ulps between the m-th and the (m + 1)-th largest key (NaN = no key); None when there is no (m + 1)-th."""
    k = np.sort(ordered(keys[~np.isnan(keys)]))[::-1]
    return None if len(k) <= m else int(k[m - 1] - k[m])


def tie_rule(keys, m):
    """The rule of include/sycl_points_amd.h (sp_weighted_sample_flags), restated on the host."""
    keys = np.asarray(keys, np.float32)
    flags = np.zeros(len(keys), np.uint8)
    cand = np.flatnonzero(~np.isnan(keys))
    if len(cand) <= m:
        flags[cand] = 1
        return flags
    K = np.sort(keys[cand])[::-1][m - 1]
    c = m - int((keys[cand] > K).sum())
    window = [i for i in cand if keys[i] >= K][:m]
    ties = [i for i in window if keys[i] == K]
    flags[[i for i in cand if keys[i] > K]] = 1
    flags[ties[len(ties) - c:]] = 1
    return flags


def random_weights(n, seed, zero_share=0.2):
    rs = np.random.RandomState(seed)
    w = rs.uniform(0.0, 1.0, n).astype(np.float32)
    w[rs.uniform(size=n) < zero_share] = 0.0
    if not (w > 0).any():
        w[0] = 0.5
    return w


def read_ply_xyzi(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int([l for l in head.split(b"\n") if l.startswith(b"element vertex")][0].split()[-1])
    return np.frombuffer(body, dtype="<f4", count=n * 4).reshape(n, 4).copy()


def golden_intensities():
    return np.ascontiguousarray(read_ply_xyzi(os.path.join(ROOT, "tests", "golden", "target.ply"))[:, 3])


def m_values(n, positive):
    """m in {1, 2, N/2, N - 1} and 1000 at the large sizes, whatever the number of positive weights (above it every positive
    weight is kept), and the two largest m that still leave a threshold among the keys: positive - 1 and positive."""
    ms = {1, 2, n // 2, n - 1, positive - 1, positive} | ({1000} if n > 4000 else set())
    return sorted(m for m in ms if 1 <= m <= n)


# The random-weight cases of the GPU suite: (n, seed of the weights and of the draws). Sizes: the wave (63, 64, 65), a few waves
# (257), one below / at / one above the kernels' tile (1023, 1024, 1025), several tiles (4097), and the golden scan (n = 0 here).
RANDOM_CASES = [(2, 1), (63, 2), (64, 3), (65, 4), (257, 5), (TILE - 1, 6), (TILE, 7), (TILE + 1, 8), (4097, 9), (0, 10)]
MARGIN_ULP = 8  # twice the 2-ulp bound between a device key and the reference's


def random_case(R, n, seed):
    """weights, draws, the restatement's keys and the m values of one random case; n == 0: the golden scan's intensities."""
    w = golden_intensities() if n == 0 else random_weights(n, seed)
    if n == 2:
        w = np.array([0.25, 0.75], np.float32)
    u = draws(R, seed, int((w > 0).sum()))
    return w, u, keys_of(R, w, u), m_values(len(w), int((w > 0).sum()))


def test_symbols_exported_and_listed(L):
    from sycl_points_amd import _lib

    names = ("sp_weight_check", "sp_weighted_sample_workspace_bytes", "sp_weighted_sample_flags",
             "sp_uniform_fill_workspace_bytes", "sp_uniform_fill_flags")
    with open(os.path.join(ROOT, "include", "sycl_points_amd.h")) as f:
        header = f.read()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(L, name) and name + "(" in header
    assert L.sp_abi_version() == 7  # the change is additive
    assert L.sp_weighted_sample_workspace_bytes(70_000) >= 4 * 70_000
    assert L.sp_uniform_fill_workspace_bytes(70_000) >= 4 * (70_000 // TILE + 2)


def test_invalid_arguments_need_no_device(L):
    from sycl_points_amd import _lib

    bad = _lib.SP_ERR_INVALID_ARGUMENT
    w = np.ones(8, np.float32)
    u = np.full(8, 0.5, np.float32)
    flags = np.zeros(8, np.uint8)
    rep = np.zeros(2, np.uint32)
    pos = np.arange(3, dtype=np.uint32)
    nb = L.sp_weighted_sample_workspace_bytes(8)
    ws = np.zeros(nb, np.uint8)
    W, U, F, REP, P, WS = (_p(a) for a in (w, u, flags, rep, pos, ws))
    for args in [(None, 8, REP), (W, 8, None), (W, 0, REP), (W, 1 << 32, REP)]:
        assert L.sp_weight_check(*args, None) == bad, args
    assert b"sp_weight_check" in L.sp_last_error()
    cases = [
        (None, U, 8, 2, F, WS, nb),       # null weights
        (W, None, 8, 2, F, WS, nb),       # null draws
        (W, U, 8, 2, None, WS, nb),       # null flags
        (W, U, 8, 2, F, None, nb),        # null workspace
        (W, U, 0, 1, F, WS, nb),          # n == 0
        (W, U, 1 << 32, 2, F, WS, 1 << 40),  # n >= 2^32
        (W, U, 8, 0, F, WS, nb),          # m == 0
        (W, U, 8, 9, F, WS, nb),          # m > n
        (W, U, 8, 2, F, WS, nb - 1),      # workspace too small
    ]
    for wp, up, n, m, fp, wsp, b in cases:
        assert L.sp_weighted_sample_flags(wp, up, n, m, fp, None, wsp, b, None) == bad, (n, m, b)
    assert b"sp_weighted_sample_flags" in L.sp_last_error()
    nb2 = L.sp_uniform_fill_workspace_bytes(8)
    cases = [
        (None, 8, P, 3, WS, nb2),         # null flags
        (F, 8, None, 3, WS, nb2),         # null positions
        (F, 8, P, 3, None, nb2),          # null workspace
        (F, 0, P, 3, WS, nb2),            # n == 0
        (F, 1 << 32, P, 3, WS, 1 << 40),  # n >= 2^32
        (F, 8, P, 0, WS, nb2),            # no positions
        (F, 8, P, 9, WS, nb2),            # more positions than points
        (F, 8, P, 3, WS, nb2 - 1),        # workspace too small
    ]
    for fp, n, pp, k, wsp, b in cases:
        assert L.sp_uniform_fill_flags(fp, n, pp, k, wsp, b, None) == bad, (n, k, b)
    assert b"sp_uniform_fill_flags" in L.sp_last_error()


def test_weighted_is_deterministic_with_seed(R):
    # WeightedRandomSamplingIsDeterministicWithSeed (:202-249)
    w = [0.1, 0.2, 0.5, 1.0, 2.0]
    rc, a = weighted_restate(R, 7, w, 3)
    rc2, b = weighted_restate(R, 7, w, 3)
    assert rc == 0 and rc2 == 0 and int(a.sum()) == 3 and np.array_equal(a, b)


def test_weighted_keeps_all_when_count_covers_input(R):
    # ...NoOpWhenSamplingCountEqualsSize / ...CopiesOutputWhenSamplingCountCoversInput (:251-310): before any check
    for m in (3, 10):
        rc, flags = weighted_restate(R, 1234, [1.0, 0.0, 2.0], m)
        assert rc == 0 and flags.tolist() == [1, 1, 1]
    assert weighted_restate(R, 1234, [-1.0, NAN], 2)[0] == 0
    assert weighted_restate(R, 1234, [], 2)[0] == 0


def test_weighted_skips_zero_weight_points(R):
    # WeightedRandomSamplingSkipsZeroWeightPoints (:312-334)
    rc, flags = weighted_restate(R, 11, [0.0, 0.0, 1.0, 2.0], 2)
    assert rc == 0 and flags.tolist() == [0, 0, 1, 1]
    for seed in range(20):
        w = random_weights(200, seed, zero_share=0.5)
        rc, flags = weighted_restate(R, seed, w, 40)
        assert rc == 0 and int(flags.sum()) == 40 and not flags[w == 0].any()


def test_weighted_checks_and_their_order(R):
    # :336-418 — 1 a weight not finite or < 0, 2 no positive weight, 3 sampling_num above the positive weights
    assert weighted_restate(R, 1234, [0.0, 0.0, 1.0, 2.0], 3)[0] == 3
    assert weighted_restate(R, 1234, [1.0, -1.0, 2.0], 2)[0] == 1
    assert weighted_restate(R, 1234, [1.0, NAN, 2.0], 2)[0] == 1
    assert weighted_restate(R, 1234, [1.0, np.inf, 2.0], 2)[0] == 1
    assert weighted_restate(R, 1234, [0.0, 0.0, 0.0], 2)[0] == 2
    assert weighted_restate(R, 1234, [0.0, -1.0, 0.0], 2)[0] == 1  # the bad weight is met before the counts are looked at


def test_mixed_ratio_zero_is_uniform_sampling(R):
    # MixedRandomSamplingMatchesUniformSamplingWhenWeightedRatioIsZero (:420-464): seed 23, 5 points, 3 samples. random_sampling's
    # partial Fisher-Yates over all indices is the uniform part with nothing selected: no weighted draw was consumed.
    rc, flags = mixed_restate(R, 23, [5.0, 4.0, 3.0, 2.0, 1.0], 3, 0.0)
    uniform = uniform_positions(R, 23, 0, 5, 3)
    assert rc == 0 and int(flags.sum()) == 3 and sorted(np.flatnonzero(flags)) == sorted(uniform.tolist())
    idx = list(range(5))  # and the same by the literal array form (random_sampling_operator.hpp:36-46), draws replayed
    for i, picked in enumerate(uniform):
        j = idx.index(int(picked))
        assert j >= i
        idx[i], idx[j] = idx[j], idx[i]
    assert sorted(idx[:3]) == sorted(uniform.tolist())


def test_mixed_falls_back_to_uniform(R):
    # MixedRandomSamplingFallsBackToUniformWhenWeightedPointsAreInsufficient (:466-494): one positive weight, target 3
    rc, flags = mixed_restate(R, 9, [1.0, 0.0, 0.0, 0.0], 3, 1.0)
    assert rc == 0 and int(flags.sum()) == 3 and flags[0] == 1 and flags[1:].any()
    # the uniform part starts after ONE weighted draw (positive_count of them, not the target)
    pos = uniform_positions(R, 9, 1, 3, 2)
    remaining = np.array([1, 2, 3])
    assert sorted(np.flatnonzero(flags)) == sorted([0] + remaining[pos.astype(int)].tolist())


def test_mixed_checks_and_their_order(R):
    # MixedRandomSamplingThrowsWhenWeightedRatioIsInvalid (:496-512): 4 the ratio, before 1 a bad weight
    for ratio in (-0.1, 1.1, float("nan"), float("inf")):
        assert mixed_restate(R, 1234, [1.0, 1.0, -1.0, 1.0], 2, ratio)[0] == 4
    assert mixed_restate(R, 1234, [1.0, 1.0, -1.0, 1.0], 2, 0.5)[0] == 1
    assert mixed_restate(R, 1234, [1.0, 1.0, -1.0, 1.0], 2, 0.0)[0] == 1  # checked even when no weighted sample is wanted
    assert mixed_restate(R, 1234, [1.0, -1.0], 2, 7.0)[0] == 0            # N <= sampling_num: before any check


def test_mixed_counts(R):
    # ...PreservesTimestampMetadataForSeparateOutput (:514-540): 3 of 5 come out; and the split in general
    rc, flags = mixed_restate(R, 31, [1.0, 0.5, 0.0, 0.0, 2.0], 3, 0.5)
    assert rc == 0 and int(flags.sum()) == 3
    w = random_weights(500, 3)
    for ratio in (0.0, 0.3, 0.8, 1.0):
        rc, flags = mixed_restate(R, 5, w, 100, ratio)
        assert rc == 0 and int(flags.sum()) == 100
        target = int(np.floor(100 * np.float64(np.float32(ratio))))
        if target:
            heap = heap_select(R, keys_of(R, w, draws(R, 5, int((w > 0).sum()))), target)
            assert not (heap & ~flags).any()  # the weighted part is the heap's, the uniform part only adds


def test_sparse_fisher_yates_matches_the_operator(R):
    """The uniform part by positions in a sparse map (sampling_uniform_positions, what the facade runs) selects what the literal
    operator selects, for U up to R."""
    for seed, n, m, ratio in [(1, 50, 20, 0.5), (2, 50, 49, 0.1), (3, 200, 150, 0.9), (4, 64, 63, 0.0), (5, 300, 299, 1.0)]:
        w = random_weights(n, seed, zero_share=0.6)
        rc, flags = mixed_restate(R, seed, w, m, float(ratio))
        assert rc == 0
        positive = int((w > 0).sum())
        target = int(np.floor(m * np.float64(np.float32(ratio))))
        mine = np.zeros(n, np.uint8)
        drawn = 0
        if target:
            mine = heap_select(R, keys_of(R, w, draws(R, seed, positive)), target)
            drawn = positive
        selected = int(mine.sum())
        assert selected == min(target, positive)
        remaining = np.flatnonzero(mine == 0)
        U = min(m - selected, len(remaining))
        pos = uniform_positions(R, seed, drawn, len(remaining), U)
        assert len(set(pos.tolist())) == U
        mine[remaining[pos.astype(int)]] = 1
        assert np.array_equal(mine, flags), (seed, n, m, ratio)


def test_keys_are_logf_over_w(R):
    u = draws(R, 1234, 1000)
    assert (u >= np.finfo(np.float32).tiny).all() and (u <= 1.0).all()
    w = np.random.RandomState(0).uniform(1e-3, 10.0, 1000).astype(np.float32)
    k = keys_of(R, w, u)
    lg = np.log(u.astype(np.float64)).astype(np.float32)  # correctly rounded but for near-ties
    assert np.abs(ordered(k) - ordered(lg / w)).max() <= 2  # glibc's logf (0.82 ulp), then one IEEE division
    assert (k <= 0).all() and not np.isnan(k).any()
    tiny = keys_of(R, np.full(4, 1e-40, np.float32), np.full(4, 0.5, np.float32))
    assert np.isneginf(tiny).all()  # a tiny (here subnormal) weight: -inf, never NaN


U9 = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9], np.float32)

# hand-made tie cases: (u per point with all weights 1, m, the indices kept), worked by the heap's rule
TIE_CASES = [
    # ties straddle the moment the heap fills: .5 .5 | .5 with m = 2: the first two fill it, the third is refused
    ([0.5, 0.5, 0.5], 2, [0, 1]),
    # a tie arrives after the heap is full of larger keys: refused
    ([0.9, 0.8, 0.5, 0.5], 3, [0, 1, 2]),
    # points above the threshold arrive after the ties and evict them, lowest index first
    ([0.5, 0.5, 0.5, 0.9], 3, [1, 2, 3]),
    ([0.5, 0.5, 0.5, 0.9, 0.8], 3, [2, 3, 4]),
    # a smaller key fills the heap first and is evicted by a tie (top.key < key), later ties are then refused
    ([0.1, 0.5, 0.5, 0.5], 2, [1, 2]),
    # the window: the first m keys >= K are 0,1,2 (ties 0 and 2); 4 evicts tie 0; tie 3 was refused
    ([0.5, 0.9, 0.5, 0.5, 0.8], 3, [1, 2, 4]),
    ([0.3, 0.5, 0.2, 0.5, 0.7, 0.5, 0.9], 3, [3, 4, 6]),
]


@pytest.mark.parametrize("u,m,kept", TIE_CASES)
def test_tie_rule_by_hand(R, u, m, kept):
    keys = keys_of(R, np.ones(len(u), np.float32), np.array(u, np.float32))
    assert np.flatnonzero(heap_select(R, keys, m)).tolist() == kept
    assert np.flatnonzero(tie_rule(keys, m)).tolist() == kept


def test_tie_rule_all_weights_one(R):
    # all weights 1 and u from {0.1 .. 0.9}: many equal keys, every m
    rs = np.random.RandomState(4)
    for n in (9, 40, 200):
        keys = keys_of(R, np.ones(n, np.float32), U9[rs.randint(0, 9, n)])
        for m in range(1, n):
            assert np.array_equal(tie_rule(keys, m), heap_select(R, keys, m)), (n, m)


def test_tie_rule_exhaustive(R):
    """Every arrangement of 8 keys from 3 values (and from 2 values and "no key"), every m: the rule equals the literal heap."""
    for values in ((-3.0, -2.0, -1.0), (-np.inf, -1.0, np.nan), (-0.0, 0.0, -1.0)):
        for arr in itertools.product(values, repeat=8):
            keys = np.array(arr, np.float32)
            for m in range(1, 9):
                assert np.array_equal(tie_rule(keys, m), heap_select(R, keys, m)), (arr, m)


def test_random_cases_have_their_margin(R):
    """The GPU suite's random cases compare a device whose keys may differ from the restatement's by 2 ulp: each case's m-th and
    (m + 1)-th largest keys are more than MARGIN_ULP apart (the GPU test asserts it again before it compares)."""
    for n, seed in RANDOM_CASES:
        w, u, keys, ms = random_case(R, n, seed)
        assert ms, (n, seed)
        for m in ms:
            gap = threshold_gap_ulp(keys, m)
            assert gap is None or gap > MARGIN_ULP, (n, seed, m, gap)
