"""The float64 yardstick for neighbour lists (test infrastructure, shared by test_oracle_kdtree_f64.py and
test_gpu_kdtree_seam.py): a plain brute force over float64 squared distances, written here and independent of the oracle,
and the properties every row of a kNN or radius search has to have against it.

Bounds, with u = 2^-24 (derived, not tuned):
  * |d - D| <= 6 u D. The fp32 distance is five roundings (three subtractions, then the squares folded into a three-step fma
    chain); csrc/knn_bruteforce.hip bounds it by 5.1 u.
  * completeness 12 u: two candidates that are each off by 6 u may swap places, so the j-th smallest D among the returned
    indices lies within a relative 12 u of the j-th smallest D of the whole cloud (cut at radius^2 for a radius search).
  * a radius search returns min(max_k, #{D <= r^2}) entries; a query with a target within 12 u of the radius is ambiguous and
    left out of the count and the completeness check (the caller bounds how many rows that may be).
"""
import numpy as np

U = 2.0 ** -24
FLT_MAX = np.finfo(np.float32).max
ERR_BOUND_U = 6.0
GAP_BOUND_U = 12.0


def matrix_cloud(orc):
    """5000 uniform targets in [-5, 5]^3 and 517 queries (a ragged last block) in [-5.5, 5.5]^3, some outside the cloud's box."""
    g = orc.rng(4242)
    return g.uniform_points(5000, 5.0), g.uniform_points(517, 5.5)


def full_leaves_size(leaf, limit=5000):
    """The largest n <= limit of the form (leaf + 1) 2^m - 1: every median split halves it exactly, so every leaf block holds
    `leaf` points and no pad slot. (On other sizes the last slots of a block are mostly pads, and a leaf loop that stopped one
    slot early would go unnoticed.)"""
    n = leaf
    while 2 * n + 1 <= limit:
        n = 2 * n + 1
    return n


def far_stack_cloud(orc):
    """300 000 uniform targets — deeper than the far stack with leaves of one or two points — and 2000 queries."""
    g = orc.rng(31)
    return g.uniform_points(300_000, 10.0), g.uniform_points(2000, 10.0)


def removals(n):
    """Flags of two lazy deletes in a row: every 7th point and a contiguous run, then every 5th of the kept points."""
    first = np.ones(n, np.uint8)
    first[::7] = 0
    first[100:900] = 0
    second = np.ones(int(first.sum()), np.uint8)
    second[::5] = 0
    return first, second


def non_finite_queries():
    """A NaN coordinate, an inf coordinate, a coordinate whose square overflows."""
    q = np.ones((3, 4), np.float32)
    q[0, 1] = np.nan
    q[1, 0] = np.inf
    q[2, 2] = 3e19
    return q


def brute_d2(q, t):
    """D[i, j] = |q_i - t_j|^2 in float64, from the fp32 coordinates as they are."""
    q64, t64 = np.asarray(q)[:, :3].astype(np.float64), np.asarray(t)[:, :3].astype(np.float64)
    D = np.zeros((len(q64), len(t64)))
    for a in range(3):  # (axis by axis: a third of the temporary of the one-line form, the same sum)
        D += (q64[:, None, a] - t64[None, :, a]) ** 2
    return D


def transformed_f64_checked(q, T, q_searched):
    """The query the search runs at is T q in fp32 (four fma roundings a coordinate: at most 4.1 u (|T| |q|)_i away from the
    float64 product). Checks `q_searched` against that bound and returns it: the yardstick then measures the search alone."""
    T64, q64 = np.asarray(T, np.float64), np.asarray(q, np.float64)
    exact = q64 @ T64.T
    mag = np.abs(q64) @ np.abs(T64).T
    assert (np.abs(q_searched[:, :3] - exact[:, :3]) <= 4.1 * U * mag[:, :3]).all()
    return q_searched


class Figures:
    """Largest figures seen by check_rows (for the log: printed by the tests, never asserted on beyond the bounds)."""

    def __init__(self):
        self.err_u = 0.0
        self.gap_u = 0.0

    def __str__(self):
        return f"max |d - D| / (u D) = {self.err_u:.3f}, max completeness gap = {self.gap_u:.3f} u"


def top_sorted(D, k):
    """The k smallest of every row of D, ascending."""
    k = min(k, D.shape[1])
    if k < D.shape[1]:
        D = np.partition(D, k - 1, axis=1)[:, :k]
    return np.sort(D, axis=1)


def gathered_d2(q, t, idx):
    """D[i, idx[i, j]] without the whole matrix (padding reads point 0)."""
    q64, t64 = np.asarray(q)[:, :3].astype(np.float64), np.asarray(t)[:, :3].astype(np.float64)
    return ((q64[:, None, :] - t64[np.where(idx < 0, 0, idx)]) ** 2).sum(2)


def check_rows(idx, d, D, radius=None, complete=True, top=None, figures=None, max_ambiguous=0.01, n=None):
    """Every row of (idx, d) — int32 / fp32, (nq, k) — against D (nq, n) float64. `radius`: a radius search (entries within
    the radius only). `complete=False`: the far stack may have dropped subtrees, so only what holds for any list is checked,
    and D may be gathered_d2(...) with the cloud's size in `n`. `top`: top_sorted(D, >= k) if the caller has it. Returns the
    number of ambiguous radius rows."""
    idx, d = np.asarray(idx), np.asarray(d)
    nq, k = idx.shape
    gathered = n is not None
    assert not (gathered and complete)
    n = n if gathered else D.shape[1]
    assert d.shape == idx.shape and D.shape[0] == nq and idx.dtype == np.int32 and d.dtype == np.float32
    pad = idx == -1
    assert ((idx >= -1) & (idx < n)).all(), "index out of range"
    assert (d[pad] == FLT_MAX).all() and (d[~pad] < FLT_MAX).all(), "padding is exactly (-1, FLT_MAX)"
    assert (pad[:, 1:] >= pad[:, :-1]).all(), "padding only at the end of a row"
    assert (d[:, 1:] >= d[:, :-1]).all(), "distances ascending"
    s = np.sort(idx, axis=1)
    assert ((s[:, 1:] != s[:, :-1]) | (s[:, 1:] == -1)).all(), "indices distinct"
    Dg = D if gathered else np.take_along_axis(D, np.where(pad, 0, idx).astype(np.int64), axis=1)
    err = np.abs(d.astype(np.float64) - Dg)
    assert (err[~pad] <= ERR_BOUND_U * U * Dg[~pad]).all(), "distance error above 6 u"
    if figures is not None and (~pad & (Dg > 0)).any():
        m = ~pad & (Dg > 0)
        figures.err_u = max(figures.err_u, float((err[m] / (U * Dg[m])).max()))
    count = (~pad).sum(1)
    if radius is not None:
        r2 = float(np.float32(radius)) ** 2
        assert (Dg[~pad] <= r2 * (1 + GAP_BOUND_U * U)).all(), "entry outside the radius"
    if not complete:
        return 0
    kk = min(k, n)
    if top is None:
        top = top_sorted(D, kk)
    top = top[:, :kk]
    if radius is None:
        ok = np.ones(nq, bool)
        want = np.full(nq, kk)
    else:
        ok = ~(np.abs(D - r2) <= GAP_BOUND_U * U * r2).any(1)
        want = np.minimum(k, (D <= r2).sum(1))
        assert (~ok).mean() <= max_ambiguous, "too many queries with a target on the radius"
    assert (count[ok] == want[ok]).all(), "number of entries"
    got = np.sort(np.where(pad, np.inf, Dg), axis=1)[:, :kk]
    live = ok[:, None] & (np.arange(kk)[None, :] < want[:, None])
    gap = np.abs(got - top)[live]
    assert (gap <= GAP_BOUND_U * U * top[live]).all(), "a nearer point is missing from the list"
    if figures is not None and (top[live] > 0).any():
        m = top[live] > 0
        figures.gap_u = max(figures.gap_u, float((gap[m] / (U * top[live][m])).max()))
    return int((~ok).sum())
