"""Engineered deep trees for csrc/bvh.hip and a host mirror of its walks (no tests in here: tests/test_bvh_walks_cpu.py and
tests/test_gpu_bvh_walks.py use it).

The clouds. cascade(D, clusters): D copies of the origin and `clusters` clusters of 20 copies of one point each, the points being
2^b on one axis and 0 elsewhere for b = 15, 14, ... and per b the axes z, y, x. In Morton order every cluster is the far side of
one level of the hierarchy and the near side is the chain down to the origin; a far side of 20 points is no leaf (kBvhLeaf = 16),
so a walk that comes down the chain with an infinite bound stacks one sibling per cluster, and log2(D / 32) more in the subtree of
the origin copies (equal keys: split by sorted position). CASCADES names the five sizes the tests use by the pushes of that
descent: 20 and 21 (the last LDS entry, the first arena entry), 46 (arena in use), 48 (both 48-entry stacks exactly full) and
50 (the heap kernel hands on, the sorted-insertion kernel overflows and scans all points).

The mirror. Tree restates the build (bounding box, Morton keys in float32, stable sort, Karras' ranges and splits with ties broken
by sorted position, child and own boxes, the lowest index below a node, the lazy delete); heap_query() restates bvh_heap_kernel
(greedy descent, the 33-point window, 20 rounds of bisection on the bit patterns, bvh_walk with the nearer child first, tie_skip
and the bound that follows the k-th (distance, index) key once k candidates are in) and sorted_query() the descent of
bvh_search_kernel (window pre-insertion for the cloud's own points, 48-entry stack, overflow). Arithmetic is float32 where the
kernels' is: fma32() is a correctly rounded float32 fused multiply-add (float64 product, round-to-odd sum, one rounding).
predict() gives, per query of one library call, the highest stack occupancy, whether an arena slot is asked for, whether the heap
kernel hands the query on and whether the sorted-insertion kernel rescans, and the two device counters of the call.

brute_force() is the expected list: (distance, index)-lexicographic over float32 dist2, for any k."""
import bisect

import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
INT_MAX = 0x7FFFFFFF
LEAF = 16           # kBvhLeaf
SEARCH_STACK = 48   # kBvhStack
LDS_STACK = 20      # kHeapStack
DEEP_STACK = 28     # kHeapStackDeep
SEL_HALF = 16       # kSelHalf
ARENA_MAX = 65536   # bvh_dispatch: min(nq, 65536) arena slots
INVALID_KEY = (1 << 48) - 1
NO_CAND = (0x7F7FFFFF << 32) | INT_MAX  # kNoCand
CLUSTER = 20
CASCADES = {20: (64, 19), 21: (64, 20), 46: (64, 45), 48: (256, 45), 50: (1024, 45)}  # pushes -> (D, clusters)


# ------------------------------------------------------------------------------------------------------------------ the clouds
def cluster_points(clusters):
    """The cluster centres in the order of the construction: b = 15 downwards, per b the axes z, y, x."""
    out = []
    for c in range(clusters):
        p = [0.0, 0.0, 0.0]
        p[2 - c % 3] = float(2 ** (15 - c // 3))
        out.append(p)
    return np.array(out, np.float32).reshape(-1, 3)


def cascade(D, clusters, seed=20240611):
    pts = np.concatenate([np.zeros((D, 3), np.float32), np.repeat(cluster_points(clusters), CLUSTER, axis=0)])
    pts = pts[np.random.RandomState(seed).permutation(len(pts))]
    return np.concatenate([pts, np.ones((len(pts), 1), np.float32)], axis=1)


def cascade_by_pushes(pushes):
    return cascade(*CASCADES[pushes])


def external_queries():
    """The origin, three points inside the first cell (the cell is 2^15 / 65535 wide), one beyond the z-15 cluster (a shallow
    walk), one of the cluster points (present in every cascade), one NaN query. Dyadic coordinates."""
    q = np.array([[0, 0, 0], [0.25, 0.125, 0.375], [0.125, 0.25, 0.0625], [0.375, 0, 0.25], [0, 0, 40000.0], [0, 4096.0, 0],
                  [np.nan, 0, 0]], np.float32)
    return np.concatenate([q, np.ones((len(q), 1), np.float32)], axis=1)


def lazy_delete_flags(cloud, count=40):
    """flags / new indices that remove the `count` origin copies with the lowest original indices."""
    origin = np.flatnonzero((cloud[:, :3] == 0).all(1))[:count]
    flags = np.ones(len(cloud), np.uint8)
    flags[origin] = 0
    new_idx = np.where(flags == 1, np.cumsum(flags) - 1, -1).astype(np.int32)
    return flags, new_idx


# ------------------------------------------------------------------------------------------------------------ float32 arithmetic
def fma32(a, b, c):
    """fmaf(a, b, c), correctly rounded: the product of two float32 is exact in float64; the sum is rounded to odd (TwoSum gives
    the error), which a final rounding to float32 turns into the single rounding of the fused operation."""
    a, b, c = (np.atleast_1d(np.asarray(v, np.float32)).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = (err != 0) & np.isfinite(s) & np.isfinite(err) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def dist2(q, pts):
    """sp_math.h dist2: fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, 0))) with d = q - t in float32. q: 3 floats, pts: (n, 3)."""
    q = np.asarray(q, np.float32)
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = q[None, :] - pts
    return fma32(d[:, 2], d[:, 2], fma32(d[:, 1], d[:, 1], fma32(d[:, 0], d[:, 0], np.zeros(len(pts), np.float32))))


def box_d2(lo, hi, q):
    """bvh.hip box_d2 for boxes lo / hi (m, 3) and the query q."""
    q = np.asarray(q, np.float32)
    with np.errstate(all="ignore"):
        g = np.fmax(np.fmax(lo - q[None, :], q[None, :] - hi), F32(0))
        return (fma32(g[:, 0], g[:, 0], fma32(g[:, 1], g[:, 1], g[:, 2] * g[:, 2])) * F32(0.999999)).astype(np.float32)


def bits(d):
    return np.asarray(d, np.float32).view(np.uint32)


# --------------------------------------------------------------------------------------------------------------------- the build
def morton_keys(pts, box):
    """bvh_key_kernel / morton_key_in_box with kBvhCells (scale 65535, clamp 65534); non-finite points get the invalid key."""
    pts = np.asarray(pts, np.float32)
    cells = np.zeros((len(pts), 3), np.uint64)
    with np.errstate(all="ignore"):
        for a in range(3):
            lo, ext = box[a], F32(box[3 + a] - box[a])
            t = (pts[:, a] - lo) / ext * F32(65535.0) if ext > 0 else np.zeros(len(pts), np.float32)
            t = np.fmin(np.fmax(t, F32(0)), F32(65534.0))
            cells[:, a] = np.where(np.isfinite(t), t, 0).astype(np.uint64)
    keys = []
    finite = np.isfinite(pts).all(1)
    for i in range(len(pts)):
        if not finite[i]:
            keys.append(INVALID_KEY)
            continue
        key = 0
        for bit in range(16):
            for a in range(3):
                key |= ((int(cells[i, a]) >> bit) & 1) << (3 * bit + a)
        keys.append(key)
    return keys


def _delta(keys, n, i, j):
    if j < 0 or j >= n:
        return -1
    a, b = keys[i], keys[j]
    return 64 + 32 - (i ^ j).bit_length() if a == b else 64 - (a ^ b).bit_length()


class Geometry:
    """What one query point sees of a tree: its float32 distances to every point and every box."""

    def __init__(self, tree, q):
        self.q = np.asarray(q, np.float32)[:3]
        self.finite = bool(np.isfinite(self.q).all())
        if not self.finite:
            return
        self.d = dist2(self.q, tree.pts)
        self.dbits = [int(b) for b in bits(self.d)]
        self.df = [float(v) for v in self.d]
        self.dl = [float(v) for v in box_d2(tree.L[:, :3], tree.L[:, 3:], self.q)]
        self.dr = [float(v) for v in box_d2(tree.R[:, :3], tree.R[:, 3:], self.q)]
        self.do = [float(v) for v in box_d2(tree.O[:, :3], tree.O[:, 3:], self.q)]


class Tree:
    def __init__(self, cloud):
        pts = np.asarray(cloud, np.float32)[:, :3]
        n = self.n = len(pts)
        finite = np.isfinite(pts).all(1)
        if finite.any():
            self.box = np.concatenate([pts[finite].min(0), pts[finite].max(0)]).astype(np.float32)
        else:
            self.box = np.array([np.inf] * 3 + [-np.inf] * 3, np.float32)
        keys = morton_keys(pts, self.box)
        order = np.argsort(np.array(keys, np.uint64), kind="stable")  # the radix sort is stable: equal keys keep their order
        self.keys = [keys[i] for i in order]
        self.pts = pts[order].copy()
        self.idx = [int(i) for i in order]  # sorted position -> index the lists report (-1: removed)
        self.first, self.split, self.last = [], [], []
        for i in range(n - 1):
            self._range(i)
        ni = max(n - 1, 0)
        self.L, self.R, self.O = (np.zeros((ni, 6), np.float32) for _ in range(3))
        self.omin = [0] * ni
        fin = finite[order]
        for i in range(ni):
            f, s, l = self.first[i], self.split[i], self.last[i]
            self.L[i], self.R[i], self.O[i] = self._box(fin, f, s), self._box(fin, s + 1, l), self._box(fin, f, l)
            self.omin[i] = min(self.idx[f:l + 1])
        self._geom = {}

    def _range(self, i):  # bvh_hierarchy_kernel
        keys, n = self.keys, self.n
        d = 1 if _delta(keys, n, i, i + 1) - _delta(keys, n, i, i - 1) >= 0 else -1
        dmin = _delta(keys, n, i, i - d)
        lmax = 2
        while _delta(keys, n, i, i + lmax * d) > dmin:
            lmax <<= 1
        l, t = 0, lmax >> 1
        while t >= 1:
            if _delta(keys, n, i, i + (l + t) * d) > dmin:
                l += t
            t >>= 1
        j = i + l * d
        dnode = _delta(keys, n, i, j)
        s, t = 0, l
        while True:
            t = (t + 1) >> 1
            if _delta(keys, n, i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
        self.split.append(i + s * d + min(d, 0))
        self.first.append(min(i, j))
        self.last.append(max(i, j))

    def _box(self, fin, f, l):
        p = self.pts[f:l + 1][fin[f:l + 1]]
        if len(p) == 0:
            return np.array([np.inf] * 3 + [-np.inf] * 3, np.float32)
        return np.concatenate([p.min(0), p.max(0)])

    def remove_by_flags(self, flags, new_idx):
        """sp_bvh_remove_by_flags: removed points stay as NaN with index -1, kept ones are relabelled, the boxes stay, the lowest
        index below a node becomes the number of kept points before it."""
        nf = len(flags)
        kept_before = np.concatenate([[0], np.cumsum(np.asarray(flags, np.int64))[:-1]])
        for c in range(self.n - 1):
            if 0 <= self.omin[c] < nf:
                self.omin[c] = int(kept_before[self.omin[c]])
        for i in range(self.n):
            o = self.idx[i]
            if o < 0 or o >= nf:
                continue
            if flags[o]:
                self.idx[i] = int(new_idx[o])
            else:
                self.pts[i] = np.nan
                self.idx[i] = -1
        self._geom = {}

    def geometry(self, q):
        key = np.asarray(q, np.float32)[:3].tobytes()
        if key not in self._geom:
            self._geom[key] = Geometry(self, q)
        return self._geom[key]

    # ---------------------------------------------------------------------------------------------- bvh_heap_kernel's first bound
    def greedy_centre(self, g):
        cur = 0
        while True:
            f, s, l = self.first[cur], self.split[cur], self.last[cur]
            left = not (g.dr[cur] < g.dl[cur])
            cf, cl = (f, s) if left else (s + 1, l)
            if cl - cf < LEAF:
                return cf + ((cl - cf) >> 1)
            cur = s if left else s + 1

    def first_bound(self, g, centre, k, top):
        """-> (bound, number of valid window positions)."""
        wb, hi, valid = [], 0, 0
        for u in range(2 * SEL_HALF + 1):
            pos = centre - SEL_HALF + u
            ok = 0 <= pos < self.n and g.dbits[pos] <= 0x7F7FFFFF
            wb.append(g.dbits[pos] if ok else 0xFFFFFFFF)
            if ok:
                hi = max(hi, g.dbits[pos])
                valid += 1
        lo = 0
        for _ in range(20):
            mid = lo + ((hi - lo) >> 1)
            if sum(1 for w in wb if w <= mid) >= k:
                hi = mid
            else:
                lo = mid + 1
        if valid >= k:
            top = min(top, float(np.array([hi], np.uint32).view(np.float32)[0]))
        return top, valid

    # -------------------------------------------------------------------------------------------------------------------- bvh_walk
    def heap_walk(self, g, k, top, lds=LDS_STACK, deep=DEEP_STACK, arena_free=True):
        """bvh_walk<lds> with the leaf function of bvh_heap_kernel. -> dict(max_stack, claimed, ok)."""
        best = []  # the k smallest keys so far, ascending (what the 4-ary heap holds, as a set)
        bound, bound_idx = top, INT_MAX
        first, split, last, omin = self.first, self.split, self.last, self.omin
        stack, max_stack, claimed, have_deep, ok = [], 0, False, False, True
        cur, have_cur, pf, pl = 0, True, 1, 0
        while have_cur or pl >= pf:
            while have_cur and pl < pf:
                f, s, l = first[cur], split[cur], last[cur]
                dl, dr = g.dl[cur], g.dr[cur]
                ll, rl = s - f < LEAF, l - (s + 1) < LEAF
                al, ar = not (dl > bound), not (dr > bound)
                if al and not ll and s > f and dl == bound and omin[s] > bound_idx:
                    al = False
                if ar and not rl and l > s + 1 and dr == bound and omin[s + 1] > bound_idx:
                    ar = False
                if al and ll:
                    pf, pl = f, s
                if ar and rl:
                    pf, pl = (f if (al and ll) else s + 1), l
                el, er = al and not ll, ar and not rl
                if el and er:
                    l_near = not (dr < dl)
                    far = s + 1 if l_near else s
                    if len(stack) < lds:
                        stack.append(far)
                    elif len(stack) < lds + deep:
                        if not have_deep:
                            claimed = True
                            have_deep = arena_free
                        if have_deep:
                            stack.append(far)
                        else:
                            ok = False
                    else:
                        ok = False
                    max_stack = max(max_stack, len(stack))
                    cur = s if l_near else s + 1
                elif el:
                    cur = s
                elif er:
                    cur = s + 1
                else:
                    have_cur = False
                    while stack:
                        c = stack.pop()
                        dc = g.do[c]
                        if dc > bound or (dc == bound and omin[c] > bound_idx):
                            continue
                        cur, have_cur = c, True
                        break
                if not ok:
                    have_cur, pf, pl, stack = False, 1, 0, []
            if pl >= pf:
                for p in range(pf, pl + 1):
                    h0 = best[-1] if len(best) == k else NO_CAND
                    nk = (g.dbits[p] << 32) | (self.idx[p] & 0xFFFFFFFF)
                    if g.df[p] <= top and nk < h0:
                        if len(best) == k:
                            best.pop()
                        bisect.insort(best, nk)
                if len(best) == k and best[-1] != NO_CAND:
                    bound = float(np.array([best[-1] >> 32], np.uint32).view(np.float32)[0])
                    bound_idx = best[-1] & 0xFFFFFFFF
                    bound_idx -= (1 << 32) if bound_idx >= (1 << 31) else 0
                pf, pl = 1, 0
        return dict(max_stack=max_stack, claimed=claimed, ok=ok)

    # ---------------------------------------------------------------------------------------------- bvh_search_kernel's descent
    def sorted_walk(self, g, k, kcap, self_pos=None, radius_sq=None, stack_cap=SEARCH_STACK):
        """-> dict(max_stack, overflow). self_pos: the sorted position of one of the cloud's own points as the query."""
        lst = []  # (distance, index) ascending, at most k
        state = dict(kth=FLT_MAX, kth_idx=-1)
        w0, w1 = 1, 0

        def scan(f, l, skip_window):
            for p in range(f, l + 1):
                if skip_window and w0 <= p <= w1:
                    continue
                d, pi = g.df[p], self.idx[p]
                if radius_sq is not None and not d <= radius_sq:
                    continue
                if d < state["kth"] or (d == state["kth"] and pi < state["kth_idx"]):
                    bisect.insort(lst, (d, pi))
                    del lst[k:]
                    if len(lst) == k:
                        state["kth"], state["kth_idx"] = lst[-1]

        if self_pos is not None and kcap > 1 and self.n > LEAF:
            half = 8 if kcap <= 10 else 16
            w0, w1 = max(self_pos - half, 0), min(self_pos + half, self.n - 1)
            scan(w0, w1, False)
        if self.n <= LEAF:
            return dict(max_stack=0, overflow=False)
        stack, max_stack, overflow, cur = [], 0, False, 0
        while True:
            f, s, l = self.first[cur], self.split[cur], self.last[cur]
            dl, dr = g.dl[cur], g.dr[cur]
            l_near = not (dr < dl)
            nxt = None
            for pas in range(2):
                take_left = (pas == 0) == l_near
                dc = dl if take_left else dr
                cf, cl = (f, s) if take_left else (s + 1, l)
                child = s if take_left else s + 1
                if dc > state["kth"] or (radius_sq is not None and dc > radius_sq):
                    continue
                if dc == state["kth"] and cl > cf and self.omin[child] > state["kth_idx"]:
                    continue
                if cl - cf < LEAF:
                    scan(cf, cl, True)
                elif nxt is None:
                    nxt = child
                elif len(stack) < stack_cap:
                    stack.append(child)
                    max_stack = max(max_stack, len(stack))
                else:
                    overflow = True
            if overflow:
                break
            if nxt is not None:
                cur = nxt
                continue
            found = False
            while stack:
                c = stack.pop()
                dc = g.do[c]
                if dc > state["kth"] or (radius_sq is not None and dc > radius_sq) or \
                        (dc == state["kth"] and self.omin[c] > state["kth_idx"]):
                    continue
                cur, found = c, True
                break
            if not found:
                break
        return dict(max_stack=max_stack, overflow=overflow)


# ------------------------------------------------------------------------------------------------------------- one library call
def heap_kcap(k):  # bvh_dispatch: (heap kernel's KCAP, the sorted-insertion kernel's behind it)
    return (5, 10) if k <= 5 else (10, 10) if k <= 10 else (21, 20) if k <= 20 else (21, 32) if k == 21 else (32, 32)


def sorted_kcap(k):
    return 1 if k == 1 else 10 if k <= 10 else 20 if k <= 20 else 32


def predict(tree, queries, k, radius=None, repeat=1):
    """One sp_bvh_search / sp_bvh_radius_search (queries: rows of >= 3 floats) or sp_bvh_self_knn (queries None) with the heap
    kernel switched on. -> (records, (handed_on, arena_claims)): a record per query with `finite`, `pushes` (the highest stack
    occupancy of bvh_walk on a stack without end; None for a non-finite query), `max_stack` (on the kernel's stack), `claimed`,
    `handed_on`, `rescan` and `valid` (window positions that counted). repeat: the query set is sent that many times over
    (the counters scale; an arena that runs out hands on the claimers that came too late)."""
    external = queries is not None
    records = []
    if not (k >= (1 if external else 2) and tree.n > LEAF):
        return records, (0, 0)
    radius_sq = None if radius is None else float(F32(radius) * F32(radius))
    rows = [(None, np.asarray(q, np.float32)[:3]) for q in queries] if external else \
           [(p, tree.pts[p]) for p in range(tree.n) if tree.idx[p] >= 0]
    for pos, q in rows:
        g = tree.geometry(q)
        rec = dict(finite=g.finite, pushes=None, max_stack=0, claimed=False, handed_on=True, rescan=False, valid=0, self_pos=pos)
        if g.finite:
            centre = tree.greedy_centre(g) if external else pos
            top, rec["valid"] = tree.first_bound(g, centre, k, FLT_MAX if radius_sq is None else radius_sq)
            w = tree.heap_walk(g, k, top)
            rec.update(max_stack=w["max_stack"], claimed=w["claimed"], handed_on=not w["ok"])
            rec["pushes"] = w["max_stack"] if w["ok"] else tree.heap_walk(g, k, top, lds=1 << 30)["max_stack"]
            if not w["ok"]:
                rec["rescan"] = tree.sorted_walk(g, k, heap_kcap(k)[1], pos, radius_sq)["overflow"]
        records.append(rec)
    nq = len(rows) * repeat
    claims = sum(r["claimed"] for r in records) * repeat
    handed = sum(r["handed_on"] for r in records) * repeat
    slots = min(nq, ARENA_MAX)
    if claims > slots:  # who comes too late depends on the order of the atomics: only a uniform set of claimers has one answer
        kinds = {r["handed_on"] for r in records if r["claimed"]}
        if len(kinds) != 1:
            raise ValueError("arena exhausted by claimers of both kinds: the handed-on count depends on their order")
        if kinds == {False}:
            handed += claims - slots
    return records, (handed, claims)


def classes(records):
    """The rare-branch classes a set of records populates."""
    out = set()
    for r in records:
        if not r["finite"]:
            continue
        if r["max_stack"] <= LDS_STACK and not r["claimed"]:
            out.add("lds")
        if r["claimed"] and not r["handed_on"]:
            out.add("arena")
        if r["max_stack"] == LDS_STACK + DEEP_STACK and not r["handed_on"]:
            out.add("full")
        if r["handed_on"]:
            out.add("handed_on")
        if r["rescan"]:
            out.add("rescan")
    return out


# ------------------------------------------------------------------------------------------------------------- the expected lists
def brute_force(queries, targets, k, radius=None):
    """(distance, index)-lexicographic brute force over float32 dist2 (a stable argsort of the distances as float64); a NaN or
    infinite distance is never a neighbour, a radius is inclusive; rows end in (-1, FLT_MAX)."""
    queries, targets = np.asarray(queries, np.float32), np.asarray(targets, np.float32)
    idx = np.full((len(queries), k), -1, np.int32)
    d2 = np.full((len(queries), k), FLT_MAX, np.float32)
    cache = {}
    for r, q in enumerate(queries[:, :3]):
        key = q.tobytes()
        if key not in cache:
            d = dist2(q, targets[:, :3]) if len(targets) else np.zeros(0, np.float32)
            ok = d < np.inf  # (NaN fails too)
            if radius is not None:
                ok &= d <= F32(radius) * F32(radius)
            order = np.argsort(np.where(ok, d, np.inf).astype(np.float64), kind="stable")
            order = order[ok[order]][:k]
            cache[key] = (order.astype(np.int32), d[order])
        oi, od = cache[key]
        idx[r, :len(oi)], d2[r, :len(oi)] = oi, od
    return idx, d2
