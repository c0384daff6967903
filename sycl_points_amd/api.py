"""Host-side mirror of the reference's operator interface for the hot path, over the C ABI.

Names, argument meaning and error behaviour follow the reference (paths relative to
/root/reference/cpp/include/sycl_points/): PointCloudShared (points/point_cloud.hpp:73-476), KNNResult
(algorithms/knn/result.hpp), KNNBase / KDTree / knn_search_bruteforce (algorithms/knn/), covariance::estimate*
(algorithms/feature/covariance.hpp), VoxelGrid (algorithms/filter/voxel_downsampling.hpp), PolarGrid
(algorithms/filter/polar_downsampling.hpp), Registration
(algorithms/registration/registration.hpp). Every array is a torch CUDA tensor resident in HBM; torch is used for
device memory, streams and torch.distributed only — all compute goes through libsycl_points_amd.so.
"""
import ctypes as C
import enum
import sys
import weakref
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from ._lib import (DegenerateRegParams, FactorParams, GnParams, Linearized, MapPriorParams, MapPriorState, SpError,
                   check)

# sp_gicp_source_prepare's sort_by_cell: False keep order / True sort per alignment / "presorted" (GridKNN.order() or
# voxel-downsampling output order): keep order, block-walk search
_SOURCE_ORDER = {False: 0, True: 1, 0: 0, 1: 1, 2: 2, "presorted": 2}
REG = {"POINT_TO_POINT": 0, "POINT_TO_PLANE": 1, "POINT_TO_DISTRIBUTION": 2, "GICP": 3, "GENZ": 4}
LOSS = {"NONE": 0, "HUBER": 1, "TUKEY": 2, "CAUCHY": 3, "GEMAN_MCCLURE": 4}
FLT_MAX = float(np.finfo(np.float32).max)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev_f32(t, cols=None):
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise SpError(1, "expected a contiguous float32 CUDA tensor")
    if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
        raise SpError(1, f"expected shape (N, {cols}), got {tuple(t.shape)}")
    return t


def _T16(T):
    """4x4 (row-major numpy / torch CPU) -> 16 floats column-major (Eigen::Matrix4f::data())."""
    a = np.ascontiguousarray(np.asarray(T, dtype=np.float32).T)
    return a


def identity():
    return np.eye(4, dtype=np.float32)


# THE list of a cloud's attribute tensors (the facade's PointCloudShared::zip): what treats every attribute alike iterates it
_CLOUD_ATTRS = ("points", "covs", "normals", "rgb", "intensities", "timestamp_offsets")


class PointCloudShared:
    """points/point_cloud.hpp:73-476 — attribute containers resident in HBM. covs are (N,16) column-major 4x4."""

    def __init__(self, points=None, covs=None, normals=None, rgb=None, intensities=None, timestamp_offsets=None,
                 device="cuda"):
        self.device = torch.device(device)
        self.points = points if points is not None else torch.empty((0, 4), dtype=torch.float32, device=self.device)
        self.covs = covs
        self.normals = normals
        self.rgb = rgb
        self.intensities = intensities
        self.timestamp_offsets = timestamp_offsets

    @staticmethod
    def from_numpy(points, device="cuda", **attrs):
        pc = PointCloudShared(torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(device), device=device)
        for k, v in attrs.items():
            if v is not None:
                setattr(pc, k, torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(device))
        return pc

    def size(self):
        return int(self.points.shape[0])

    def reordered(self, perm):
        """A copy with every attribute gathered through `perm` (e.g. GridKNN.order())."""
        return PointCloudShared(device=self.device, **{k: t[perm].contiguous() for k in _CLOUD_ATTRS
                                                       if (t := getattr(self, k)) is not None})

    def has_cov(self):
        return self.covs is not None and self.covs.shape[0] == self.points.shape[0]

    def has_normal(self):
        return self.normals is not None and self.normals.shape[0] == self.points.shape[0]

    def has_rgb(self):
        return self.rgb is not None and self.rgb.shape[0] == self.points.shape[0]

    def has_intensity(self):
        return self.intensities is not None and self.intensities.shape[0] == self.points.shape[0]

    def has_timestamps(self):
        return (self.timestamp_offsets is not None and self.timestamp_offsets.shape[0] == self.points.shape[0]
                and self.points.shape[0] > 0)


@dataclass
class KNNResult:
    """algorithms/knn/result.hpp:12-34 — row-major (query_size, k), squared distances, -1 / FLT_MAX padding."""
    indices: torch.Tensor = None
    distances: torch.Tensor = None
    query_size: int = 0
    k: int = 0

    def allocate(self, query_size, k, device="cuda"):
        self.query_size, self.k = query_size, k
        self.indices = torch.full((query_size, k), -1, dtype=torch.int32, device=device)
        self.distances = torch.full((query_size, k), FLT_MAX, dtype=torch.float32, device=device)

    def resize(self, query_size, k, device="cuda"):
        """result.resize(query_size, k) (result.hpp:28-33); reallocates only when the shape changes."""
        if self.indices is None or tuple(self.indices.shape) != (query_size, k) or self.indices.device != torch.device(device):
            self.allocate(query_size, k, device)
        self.query_size, self.k = query_size, k


def _points_of(q):
    return q.points if isinstance(q, PointCloudShared) else q


def knn_search_bruteforce(queries, targets, k):
    """algorithms/knn/bruteforce.hpp:24-96 (synchronous in the reference; here enqueued on the current stream)."""
    q = _dev_f32(_points_of(queries), 4)
    t = _dev_f32(_points_of(targets), 4)
    L = _lib.lib()
    res = KNNResult()
    res.allocate(q.shape[0], k, q.device)
    nbytes = L.sp_knn_bruteforce_workspace_bytes(q.shape[0], t.shape[0], k)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=q.device)
    check(L.sp_knn_bruteforce(_ptr(q), q.shape[0], _ptr(t), t.shape[0], k, _ptr(res.indices), _ptr(res.distances),
                              _ptr(ws), nbytes, _stream()))
    return res


def _trans_arg(transT):
    """-> (pointer, on_device flag, keepalive). Accepts None, a 4x4 host matrix, or a 16-float CUDA tensor
    (column-major) for device-resident loops."""
    if transT is None:
        return None, 0, None
    if isinstance(transT, torch.Tensor) and transT.is_cuda:
        if transT.numel() != 16 or transT.dtype != torch.float32:
            raise SpError(1, "device transT must be 16 float32 (column-major)")
        return _ptr(transT), 1, transT
    a = _T16(transT.cpu().numpy() if isinstance(transT, torch.Tensor) else transT)
    return a.ctypes.data_as(C.c_void_p), 0, a


class KNNBase:
    """algorithms/knn/knn.hpp:14-61 — the operator boundary Registration::align sits on."""

    def knn_search_async(self, queries, k, result, transT=None):
        raise NotImplementedError

    def _knn_search(self, entry, limit, too_large, queries, k, result, transT, own=()):
        """knn_search_async of a structure behind the C ABI: `entry` is its sp_*_search, `limit` its longest list and `too_large`
        its own error text; `own`: what sp_knn_tree_search takes between the pose and the outputs."""
        q = _dev_f32(_points_of(queries), 4)
        if k > limit:
            raise SpError(2, too_large)
        result.resize(q.shape[0], k, q.device)
        if q.shape[0] == 0:
            return
        tp, on_dev, keep = _trans_arg(transT)
        check(entry(self._h, _ptr(q), q.shape[0], k, tp, on_dev, *own, _ptr(result.indices), _ptr(result.distances), _stream()))

    def _radius_search(self, entry, limit, too_large, queries, max_k, radius, result, transT):
        """radius_search_async likewise, over sp_*_radius_search."""
        q = _dev_f32(_points_of(queries), 4)
        if max_k > limit:
            raise SpError(2, too_large)
        if q.shape[0] == 0 or max_k == 0:
            result.resize(0, 0, q.device)
            return
        result.resize(q.shape[0], max_k, q.device)
        tp, on_dev, keep = _trans_arg(transT)
        check(entry(self._h, _ptr(q), q.shape[0], max_k, radius, tp, on_dev, _ptr(result.indices), _ptr(result.distances), _stream()))

    def knn_search(self, queries, k, transT=None):
        r = KNNResult()
        self.knn_search_async(queries, k, r, transT)
        torch.cuda.current_stream().synchronize()
        return r

    def nearest_neighbor_search_async(self, queries, result, transT=None):
        return self.knn_search_async(queries, 1, result, transT)

    def nearest_neighbor_search(self, queries, result, transT=None):
        self.nearest_neighbor_search_async(queries, result, transT)
        torch.cuda.current_stream().synchronize()


class KDTree(KNNBase):
    """algorithms/knn/kdtree.hpp:142-766. build(points) is the reference's tree (host build with its rule, device search).
    build(points, accelerate=True) is the library's sp_knn_tree, which the C++ facade's KDTree wraps too: its own copy of the
    points and, per search, the structure csrc/knn_tree.hip chooses (`backend_for`: that choice, without searching)."""

    _BACKENDS = ("kdtree", "bvh", "grid", "bruteforce")  # SP_KNN_HOST_TREE, SP_KNN_HIERARCHY, SP_KNN_GRID, SP_KNN_BRUTE_FORCE
    _INFO = {"size": 0, "pristine": 1, "hierarchy_built": 2, "grid_built": 3}  # SP_KNN_TREE_*

    def __init__(self, handle, n, device, built_on=None):
        self._h = handle
        self.n = n
        self.device = device
        self._accelerated = built_on is not None
        self._built_on = built_on  # accelerate=True: (weak reference to the points tensor, its _version at build())

    @staticmethod
    def build(points, leaf_threshold=16, accelerate=False):
        p = _points_of(points)
        h = C.c_void_p()
        if accelerate:
            pd = _dev_f32(p, 4)
            check(_lib.lib().sp_knn_tree_create(_ptr(pd), pd.shape[0], leaf_threshold, _stream(), C.byref(h)))
            return KDTree(h, pd.shape[0], pd.device, (weakref.ref(pd), pd._version))
        host = np.ascontiguousarray(p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else p, np.float32)
        dev = p.device if isinstance(p, torch.Tensor) and p.is_cuda else torch.device("cuda")
        check(_lib.lib().sp_kdtree_create(host.ctypes.data_as(C.c_void_p), host.shape[0], leaf_threshold, _stream(),
                                          C.byref(h)))
        return KDTree(h, host.shape[0], dev)

    def _fn(self, name):
        return getattr(_lib.lib(), ("sp_knn_tree_" if self._accelerated else "sp_kdtree_") + name)

    def _own_cloud(self, q):
        """The queries are the tensor the tree was built on (same storage, length and version): sp_knn_tree's own_cloud."""
        t = self._built_on[0]()
        return int(t is not None and isinstance(q, torch.Tensor) and q.is_cuda and q.shape[0] == self.n and
                   q.data_ptr() == t.data_ptr() and t._version == self._built_on[1])

    def _info(self, what):  # sp_knn_tree_info (accelerate=True), `what` a key of _INFO
        v = C.c_uint64()
        check(_lib.lib().sp_knn_tree_info(self._h, KDTree._INFO[what], C.byref(v)))
        return int(v.value)

    def backend_for(self, queries, k, transT=None):
        """'kdtree' | 'bvh' | 'grid' | 'bruteforce': what knn_search_async(queries, k, ..., transT) answers from
        (sp_knn_tree_backend)."""
        if not self._accelerated:
            return "kdtree"
        q = _points_of(queries)
        tp, on_dev, keep = _trans_arg(transT)
        b = C.c_int()
        check(_lib.lib().sp_knn_tree_backend(self._h, q.shape[0], k, tp, on_dev, self._own_cloud(q), _stream(), C.byref(b)))
        return KDTree._BACKENDS[b.value]

    def __del__(self):
        try:
            if self._h:
                self._fn("destroy")(self._h)
                self._h = None
        except Exception:
            pass

    def knn_search_async(self, queries, k, result, transT=None):
        q = _dev_f32(_points_of(queries), 4)
        own = (self._own_cloud(q),) if self._accelerated else ()
        self._knn_search(self._fn("search"), 100, "[KDTree::knn_search_async] `k` is too large. not support.", q, k, result, transT, own)

    def radius_search_async(self, queries, max_k, radius, result, transT=None):
        self._radius_search(self._fn("radius_search"), 100, "[KDTree::radius_search_async] `max_k` is too large. not support.",
                            queries, max_k, radius, result, transT)

    def remove_nodes_by_flags(self, flags, indices):
        if flags.shape[0] != indices.shape[0]:
            raise SpError(2, "[KDTree::remove_nodes_by_flags_impl] flags and indices must have the same size.")
        check(self._fn("remove_by_flags")(self._h, _ptr(flags), _ptr(indices), flags.shape[0], _stream()))
        torch.cuda.current_stream().synchronize()


class BVH(KNNBase):
    """MI355X-native KNNBase for clouds of any density profile (csrc/bvh.hip): a bounding-volume hierarchy over the
    Morton-sorted points, built entirely on the device (the job of KDTree::build, kdtree.hpp:292-413, without its host
    build); exact kNN, k <= 32, bit-identical to knn_search_bruteforce."""

    def __init__(self, handle, n, device):
        self._h = handle
        self.n = n
        self.device = device

    @staticmethod
    def build(points):
        p = _dev_f32(_points_of(points), 4)
        h = C.c_void_p()
        check(_lib.lib().sp_bvh_create(_ptr(p), p.shape[0], _stream(), C.byref(h)))
        return BVH(h, p.shape[0], p.device)

    def __del__(self):
        try:
            if self._h:
                _lib.lib().sp_bvh_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def knn_search_async(self, queries, k, result, transT=None):
        self._knn_search(_lib.lib().sp_bvh_search, 32, "[BVH::knn_search_async] `k` is too large. not support.", queries, k, result,
                         transT)

    def _set_option(self, name, value):
        """csrc/sp_internal.h switches of this handle (tests, comparisons)."""
        check(_lib.lib().sp_internal_bvh_option(self._h, _lib.INTERNAL_OPTION[name], int(value)))

    def _walk_counts(self):
        """(queries handed on to the sorted-insertion kernel, arena slots asked for) of the last search, which ran with
        _set_option("bvh_walk_counts", 1): sp_internal_bvh_walk_counts (waits for that search)."""
        handed, claims = C.c_uint32(), C.c_uint32()
        check(_lib.lib().sp_internal_bvh_walk_counts(self._h, C.byref(handed), C.byref(claims)))
        return int(handed.value), int(claims.value)

    def self_knn(self, k):
        """The cloud's own points as queries, in tree order (row i = neighbours of point i)."""
        res = KNNResult()
        res.resize(self.n, k, self.device)
        if self.n:
            check(_lib.lib().sp_bvh_self_knn(self._h, k, _ptr(res.indices), _ptr(res.distances), _stream()))
        return res

    def radius_search_async(self, queries, max_k, radius, result, transT=None):
        """KDTree::radius_search_async (kdtree.hpp:574-719) on the device-built hierarchy (sp_bvh_radius_search), max_k <= 32."""
        self._radius_search(_lib.lib().sp_bvh_radius_search, 32, "[BVH::radius_search_async] `max_k` is too large (max 32).", queries,
                            max_k, radius, result, transT)

    def radius_search(self, queries, max_k, radius, transT=None):
        r = KNNResult()
        self.radius_search_async(queries, max_k, radius, r, transT)
        torch.cuda.current_stream().synchronize()
        return r

    def remove_nodes_by_flags(self, flags, indices):
        """KDTree::remove_nodes_by_flags (kdtree.hpp:721-765), lazily: sp_bvh_remove_by_flags."""
        if flags.shape[0] != indices.shape[0]:
            raise SpError(2, "[BVH::remove_nodes_by_flags] flags and indices must have the same size.")
        check(_lib.lib().sp_bvh_remove_by_flags(self._h, _ptr(flags), _ptr(indices), flags.shape[0], _stream()))


class Octree(KNNBase):
    """algorithms/knn/octree.hpp:27-844 on a device-built octree (csrc/octree.hip, sp_octree_*): exact kNN for k <= 100, rows
    bit-identical to knn_search_bruteforce (ties to the lowest index), lazy removal."""

    _INFO = {"nodes": 0, "leaves": 1, "depth": 2, "next_id": 3, "slots": 4}  # SP_OCTREE_*

    def __init__(self, handle, device, resolution, max_points_per_node):
        self._h = handle
        self.device = device
        self.resolution = resolution
        self.max_points_per_node = max_points_per_node

    @staticmethod
    def build(points, resolution, max_points_per_node=32):
        p = _dev_f32(_points_of(points), 4)
        h = C.c_void_p()
        check(_lib.lib().sp_octree_create(_ptr(p), p.shape[0], resolution, max_points_per_node, _stream(), C.byref(h)))
        return Octree(h, p.device, resolution, max_points_per_node)

    def __del__(self):
        try:
            if self._h:
                _lib.lib().sp_octree_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def size(self):
        return int(_lib.lib().sp_octree_size(self._h))

    def info(self, what):
        """sp_octree_info: 'nodes' | 'leaves' | 'depth' | 'next_id' | 'slots'."""
        v = C.c_uint64()
        check(_lib.lib().sp_octree_info(self._h, Octree._INFO[what], C.byref(v)))
        return int(v.value)

    def knn_search_async(self, queries, k, result, transT=None):
        q = _dev_f32(_points_of(queries), 4)
        if k > 100:  # octree.hpp:629
            raise SpError(2, "[Octree::knn_search_async] Requested neighbor count exceeds the supported maximum")
        result.resize(q.shape[0], k, q.device)
        if q.shape[0] == 0 or k == 0:  # octree.hpp:603-611
            return
        tp, on_dev, keep = _trans_arg(transT)
        check(_lib.lib().sp_octree_search(self._h, _ptr(q), q.shape[0], k, tp, on_dev, _ptr(result.indices),
                                          _ptr(result.distances), _stream()))

    def remove_nodes_by_flags(self, flags, indices):
        """octree.hpp:276-380: flags 1 = keep, a kept point p is relabelled indices[p]."""
        if flags.shape[0] != indices.shape[0]:
            raise SpError(2, "[Octree::remove_nodes_by_flags] flags and indices must have the same size")
        check(_lib.lib().sp_octree_remove_by_flags(self._h, _ptr(flags), _ptr(indices), flags.shape[0], _stream()))

    def export(self):
        """(nodes, ids) as numpy arrays: nodes is (n_nodes, 16) int32 — words 0-5 the float bits of the box (min xyz, max xyz),
        6 is_leaf, 7 depth, 8-15 the child indices (-1: none) or start, count and zeros; ids the stored ids in leaf order."""
        nodes = torch.empty((self.info("nodes"), 16), dtype=torch.int32, device=self.device)
        ids = torch.empty((self.info("slots"),), dtype=torch.int32, device=self.device)
        check(_lib.lib().sp_octree_export(self._h, _ptr(nodes), _ptr(ids), _stream()))
        torch.cuda.current_stream().synchronize()
        return nodes.cpu().numpy(), ids.cpu().numpy()


class GridKNN(KNNBase):
    """MI355X-native KNNBase: exact kNN on a device-built uniform grid (csrc/grid.hip); bit-identical to
    knn_search_bruteforce. `points_per_cell` tunes the cell size (about 2 for k = 1, about 6-8 for k = 20)."""

    def __init__(self, handle, n, device):
        self._h = handle
        self.n = n
        self.device = device

    @staticmethod
    def build(points, cell_size=0.0, points_per_cell=2.0, adaptive=False, bounds=None):
        """adaptive: the cell size follows the measured occupancy (sp_grid_create_adaptive) — clouds of surfaces.
        bounds: (min x, y, z, max x, y, z) of a box the caller knows to hold every finite point (sp_grid_create_bounded: no
        bounding-box kernel, no read-back)."""
        p = _dev_f32(_points_of(points), 4)
        h = C.c_void_p()
        if bounds is not None:
            b = (C.c_float * 6)(*[float(v) for v in bounds])
            check(_lib.lib().sp_grid_create_bounded(_ptr(p), p.shape[0], b, cell_size, points_per_cell, _stream(), C.byref(h)))
        elif adaptive:
            check(_lib.lib().sp_grid_create_adaptive(_ptr(p), p.shape[0], points_per_cell, _stream(), C.byref(h)))
        else:
            check(_lib.lib().sp_grid_create(_ptr(p), p.shape[0], cell_size, points_per_cell, _stream(), C.byref(h)))
        return GridKNN(h, p.shape[0], p.device)

    def _set_option(self, name, value):
        """csrc/sp_internal.h tuning switch of this grid (tests / scratch only)."""
        check(_lib.lib().sp_internal_grid_option(self._h, _lib.INTERNAL_OPTION[name], int(value)))

    def cell_size(self):
        return float(_lib.lib().sp_grid_cell_size(self._h))

    def max_cell_points(self):
        """Points in the fullest cell at build time (sp_grid_max_cell_points): far above the points-per-cell target means the
        cloud is not of near-uniform density and a BVH serves it better."""
        return int(_lib.lib().sp_grid_max_cell_points(self._h))

    def order(self):
        """Original indices of the points in this grid's cell order (int64 tensor, usable for tensor indexing). A source
        cloud stored in this order needs no per-alignment sort (align_fused_loop(sort_by_cell="presorted"))."""
        out = torch.empty(self.n, dtype=torch.int32, device=self.device)
        check(_lib.lib().sp_grid_order(self._h, _ptr(out), _stream()))
        return out.long()

    def __del__(self):
        try:
            if self._h:
                _lib.lib().sp_grid_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def self_knn(self, k, want_knn=True, want_covs=False, want_normals=False):
        """kNN of the grid's own cloud (the self-kNN kernels of csrc/grid.hip, chosen by k) with covariance / normal estimation optionally
        fused in — covariance::estimate_async(knn, points, k) (covariance.hpp:305-311) when the KNNBase is a GridKNN
        built on `points`. Returns (KNNResult | None, covs | None, normals | None), rows in original point order."""
        if k > 20:
            raise SpError(2, "[GridKNN::knn_search_async] `k` is too large (max 20).")
        L = _lib.lib()
        dev = self.device
        res = None
        if want_knn:
            res = KNNResult()
            res.allocate(self.n, k, dev)
        covs = torch.empty((self.n, 16), dtype=torch.float32, device=dev) if want_covs else None
        nrm = torch.empty((self.n, 4), dtype=torch.float32, device=dev) if want_normals else None
        nbytes = L.sp_grid_self_workspace_bytes(self._h)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        check(L.sp_grid_self_knn(self._h, k, _ptr(res.indices) if res else None, _ptr(res.distances) if res else None,
                                 _ptr(covs), _ptr(nrm), _ptr(ws), nbytes, _stream()))
        self._keep = ws
        return res, covs, nrm

    def covariances_sharded(self, k, rank, world, all_gather):
        """The pre-loop of a multi-GPU run sharded by query: this rank computes the k-neighbour covariances
        of the grid positions [rank * c, (rank + 1) * c), c = ceil(n / world) (sp_grid_self_knn_range), the chunks — made
        contiguous by sp_grid_gather_rows — are exchanged by `all_gather(send, recv)` (Communicator.all_gather, or a
        torch.distributed all_gather_into_tensor), and sp_grid_scatter_rows puts all n rows back into the cloud's order.
        Bit-identical to self_knn(k, want_covs=True) of the whole cloud."""
        L = _lib.lib()
        dev = self.device
        n = self.n
        c = (n + world - 1) // world
        first = min(rank * c, n)
        count = min(c, n - first)
        covs = torch.empty((n, 16), dtype=torch.float32, device=dev)
        nbytes = L.sp_grid_self_workspace_bytes(self._h)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        check(L.sp_grid_self_knn_range(self._h, k, first, count, None, None, _ptr(covs), None, _ptr(ws), nbytes, _stream()))
        send = torch.zeros((c, 16), dtype=torch.float32, device=dev)  # equal chunks; the last rank's tail stays zero
        check(L.sp_grid_gather_rows(self._h, _ptr(covs), 64, first, count, _ptr(send), _stream()))
        recv = torch.empty((world * c, 16), dtype=torch.float32, device=dev)
        all_gather(send, recv)
        check(L.sp_grid_scatter_rows(self._h, _ptr(recv), 64, 0, n, _ptr(covs), _stream()))
        self._keep = (ws, send, recv)
        return covs

    def knn_search_async(self, queries, k, result, transT=None):
        self._knn_search(_lib.lib().sp_grid_search, 20, "[GridKNN::knn_search_async] `k` is too large (max 20).", queries, k, result,
                         transT)

    def radius_search_async(self, queries, max_k, radius, result, transT=None):
        """The grid's counterpart of KDTree::radius_search_async (kdtree.hpp:251-280): the max_k nearest within radius."""
        self._radius_search(_lib.lib().sp_grid_radius_search, 20, "[GridKNN::radius_search_async] `max_k` is too large (max 20).",
                            queries, max_k, radius, result, transT)

    def radius_search(self, queries, max_k, radius, transT=None):
        result = KNNResult()
        self.radius_search_async(queries, max_k, radius, result, transT)
        return result

    def remove_nodes_by_flags(self, flags, indices):
        """The grid's counterpart of KDTree::remove_nodes_by_flags (kdtree.hpp:282-284): flags 1 = keep; kept point p is
        relabelled indices[p]. Prepared targets built on this grid must be re-created."""
        if flags.shape[0] != indices.shape[0]:
            raise SpError(2, "[GridKNN::remove_nodes_by_flags] flags and indices must have the same size.")
        check(_lib.lib().sp_grid_remove_by_flags(self._h, _ptr(flags), _ptr(indices), flags.shape[0], _stream()))
        self.n = int(_lib.lib().sp_grid_size(self._h))


class BruteForceKNN(KNNBase):
    """A KNNBase over knn_search_bruteforce (the reference tests inject such host fakes through the same seam,
    tests/test_registration_pipeline.cpp:16-61). The query transform is applied with sp_transform first."""

    def __init__(self, targets):
        self.targets = _dev_f32(_points_of(targets), 4)

    def knn_search_async(self, queries, k, result, transT=None):
        q = _dev_f32(_points_of(queries), 4)
        if transT is not None:
            if isinstance(transT, torch.Tensor) and transT.is_cuda:
                transT = transT.cpu().numpy().reshape(4, 4).T
            q = transform_points(q, transT)
        r = knn_search_bruteforce(q, self.targets, k)
        result.indices, result.distances, result.query_size, result.k = r.indices, r.distances, r.query_size, r.k


# ------------------------------------------------------------------ covariance / normals
class covariance:
    """algorithms/feature/covariance.hpp"""

    @staticmethod
    def estimate(neighbors, points):
        """estimate_async (covariance.hpp:260-311): returns (N,16) column-major covariances."""
        p = _dev_f32(_points_of(points), 4)
        idx = neighbors.indices if isinstance(neighbors, KNNResult) else neighbors
        covs = torch.empty((p.shape[0], 16), dtype=torch.float32, device=p.device)
        check(_lib.lib().sp_cov_estimate(_ptr(p), p.shape[0], _ptr(idx), idx.shape[1] if idx.dim() == 2 else 0,
                                         _ptr(covs), _stream()))
        if isinstance(points, PointCloudShared):
            points.covs = covs
        return covs

    @staticmethod
    def estimate_robust(neighbors, points, robust_type="CAUCHY", mad_scale=1.0, min_robust_scale=1.0,
                        robust_max_iterations=1):
        """estimate_robust_async (covariance.hpp:323-381): M-estimated covariances, same layout as estimate()."""
        p = _dev_f32(_points_of(points), 4)
        idx = neighbors.indices if isinstance(neighbors, KNNResult) else neighbors
        covs = torch.empty((p.shape[0], 16), dtype=torch.float32, device=p.device)
        check(_lib.lib().sp_cov_estimate_robust(_ptr(p), p.shape[0], _ptr(idx), idx.shape[1] if idx.dim() == 2 else 0,
                                                LOSS[robust_type], mad_scale, min_robust_scale, robust_max_iterations,
                                                _ptr(covs), _stream()))
        if isinstance(points, PointCloudShared):
            points.covs = covs
        return covs

    @staticmethod
    def normalize_covariance(covs):
        """kernel::normalize_covariance over an array (covariance.hpp:76-95)"""
        out = torch.empty_like(covs)
        check(_lib.lib().sp_cov_normalize(_ptr(covs), covs.shape[0], _ptr(out), _stream()))
        return out

    @staticmethod
    def estimate_normals(neighbors, points):
        """estimate_normals_async (covariance.hpp:417-459)"""
        p = _dev_f32(_points_of(points), 4)
        idx = neighbors.indices if isinstance(neighbors, KNNResult) else neighbors
        nrm = torch.empty((p.shape[0], 4), dtype=torch.float32, device=p.device)
        check(_lib.lib().sp_normals_from_knn(_ptr(p), p.shape[0], _ptr(idx), idx.shape[1], _ptr(nrm), _stream()))
        if isinstance(points, PointCloudShared):
            points.normals = nrm
        return nrm

    @staticmethod
    def extract_normals(points, covs=None):
        """extract_normals_async (covariance.hpp:465-503)"""
        p = _dev_f32(_points_of(points), 4)
        c = covs if covs is not None else (points.covs if isinstance(points, PointCloudShared) else None)
        if c is None:
            raise SpError(2, "[covariance::extract_normals_async] covariances not computed")
        nrm = torch.empty((p.shape[0], 4), dtype=torch.float32, device=p.device)
        check(_lib.lib().sp_normals_from_cov(_ptr(p), _ptr(c), p.shape[0], _ptr(nrm), _stream()))
        if isinstance(points, PointCloudShared):
            points.normals = nrm
        return nrm

    @staticmethod
    def update_covariance_plane(covs):
        """kernel::update_covariance_plane over an array (covariance.hpp:67-74)"""
        out = torch.empty_like(covs)
        check(_lib.lib().sp_cov_update_plane(_ptr(covs), covs.shape[0], _ptr(out), _stream()))
        return out


# ------------------------------------------------------------------ global registration (MI355X extension)
def _ws_bytes(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)

# ------------------------------------------------------------------ photometric term (MI355X extension)
@dataclass
class PhotometricParams:
    """RegistrationParams::photometric (the reference has no such field): weight 0 switches the term off."""
    weight: float = 0.0
    robust_type: str = "NONE"
    robust_scale: float = 1.0

    def c_struct(self, max_correspondence_distance):
        return _lib.PhotometricParams(self.weight, LOSS[self.robust_type], self.robust_scale, max_correspondence_distance)


def intensity_gradients(neighbors, cloud):
    """feature::compute_intensity_gradients_async (sp_intensity_gradient): one row (d.x, d.y, d.z, I) per point of `cloud` from a kNN
    result of the cloud on itself (k >= 2): the intensity's gradient in the point's tangent plane and the intensity itself;
    (0, 0, 0, NaN) where there is none. The cloud needs unit normals and intensities. The gradients are in the frame the cloud is
    in now: transform the cloud and they are stale."""
    p = _dev_f32(cloud.points, 4)
    if not cloud.has_normal():
        raise SpError(2, "[feature::compute_intensity_gradients_async] normals not computed")
    if not cloud.has_intensity():
        raise SpError(2, "[feature::compute_intensity_gradients_async] the cloud has no intensities")
    nrm, inten = _dev_f32(cloud.normals, 4), _dev_f32(cloud.intensities)
    idx = neighbors.indices if isinstance(neighbors, KNNResult) else neighbors
    n, k = p.shape[0], int(idx.shape[1]) if idx.dim() == 2 else 0
    rows = torch.empty((n, 4), dtype=torch.float32, device=p.device)
    check(_lib.lib().sp_intensity_gradient(_ptr(p), _ptr(nrm), _ptr(inten), n, _ptr(idx), k, _ptr(rows), _stream()))
    return rows


def _photometric(entry, source, target_points, target_rows, neighbors, transT, params, max_correspondence_distance, lin, rows, ws):
    L = _lib.lib()
    src, inten = _dev_f32(source.points, 4), _dev_f32(source.intensities)
    pp = params.c_struct(max_correspondence_distance)
    tp, on_dev, keep = _trans_arg(transT)
    if ws is None:
        ws = _ws_bytes(L.sp_photometric_workspace_bytes(src.shape[0]), src.device)
    if lin is None:
        lin = torch.zeros(48, dtype=torch.float32, device=src.device)
    head = (_ptr(src), _ptr(inten), src.shape[0], _ptr(_dev_f32(target_points, 4)), _ptr(_dev_f32(target_rows, 4)),
            _ptr(neighbors.indices), _ptr(neighbors.distances), tp, on_dev, C.byref(pp), _ptr(lin))
    if entry == "linearize":
        check(L.sp_photometric_linearize(*head, _ptr(rows), _ptr(ws), ws.numel(), _stream()))
    else:
        check(L.sp_photometric_error(*head, _ptr(ws), ws.numel(), _stream()))
    return lin


def photometric_linearize(source, target_points, target_rows, neighbors, transT, params, max_correspondence_distance, want_rows=False,
                          lin=None, workspace=None):
    """sp_photometric_linearize over a k = 1 KNNResult of `source` (points + intensities) in the target: the 192-byte system (a
    48-float device tensor, the sp_linearized layout; params.weight NOT applied) and, with want_rows, every point's 28 values."""
    rows = torch.empty((source.size(), 28), dtype=torch.float32, device=source.points.device) if want_rows else None
    lin = _photometric("linearize", source, target_points, target_rows, neighbors, transT, params, max_correspondence_distance, lin,
                       rows, workspace)
    return (lin, rows) if want_rows else lin


def photometric_error(source, target_points, target_rows, neighbors, transT, params, max_correspondence_distance, lin=None,
                      workspace=None):
    """sp_photometric_error: the term's robust error and the count of contributing points over the same inputs."""
    return _photometric("error", source, target_points, target_rows, neighbors, transT, params, max_correspondence_distance, lin, None,
                        workspace)



def fpfh(neighbors, cloud, want_counts=False):
    """feature::compute_fpfh_async (MI355X extension; sp_fpfh_compute): one FPFH row of 36 floats (33 bins, 3 zeros) per point of
    `cloud` from a kNN result of the cloud on itself (k <= 64). The cloud's normals must be of unit length and consistently
    oriented (covariance.estimate_normals on a sensor-centred scan). want_counts: also the SPFH counts (n, 33) and m (n,) as
    int32 tensors."""
    p = _dev_f32(cloud.points, 4)
    if not cloud.has_normal():
        raise SpError(2, "[feature::compute_fpfh_async] normals not computed")
    nrm = _dev_f32(cloud.normals, 4)
    idx, d2 = neighbors.indices, neighbors.distances
    n, k = p.shape[0], int(idx.shape[1]) if idx.dim() == 2 else 0
    L = _lib.lib()
    out = torch.empty((n, _lib.FPFH_STRIDE), dtype=torch.float32, device=p.device)
    counts = torch.zeros((n, _lib.FPFH_BINS), dtype=torch.int16, device=p.device) if want_counts else None
    m = torch.zeros(n, dtype=torch.int16, device=p.device) if want_counts else None
    nbytes = L.sp_fpfh_workspace_bytes(n)
    ws = _ws_bytes(nbytes, p.device)
    check(L.sp_fpfh_compute(_ptr(p), _ptr(nrm), n, _ptr(idx), _ptr(d2), k, _ptr(out), _ptr(counts), _ptr(m), _ptr(ws), ws.numel(),
                            _stream()))
    if want_counts:  # (uint16 on the device)
        return out, counts.to(torch.int32) & 0xFFFF, m.to(torch.int32) & 0xFFFF
    return out


def _feature_rows(t):
    t = _dev_f32(t)
    if t.dim() != 2 or t.shape[1] != _lib.FPFH_STRIDE:
        raise SpError(1, f"expected descriptor rows of shape (N, {_lib.FPFH_STRIDE}), got {tuple(t.shape)}")
    return t


def match_features(a, b):
    """registration::match_features (sp_feature_match): for every row of `a` the nearest row of `b` over the 33 bins ->
    (indices int32, squared distances); -1 / FLT_MAX for an empty b; ties to the lowest index."""
    a, b = _feature_rows(a), _feature_rows(b)
    L = _lib.lib()
    na, nb = a.shape[0], b.shape[0]
    idx = torch.empty(na, dtype=torch.int32, device=a.device)
    d2 = torch.empty(na, dtype=torch.float32, device=a.device)
    ws = _ws_bytes(L.sp_feature_match_workspace_bytes(na, nb), a.device)
    check(L.sp_feature_match(_ptr(a), na, _ptr(b), nb, _ptr(idx), _ptr(d2), _ptr(ws), ws.numel(), _stream()))
    return idx, d2


def match_features_mutual(src, tgt):
    """sp_feature_match_mutual: the (i, j) pairs with j the nearest row of `tgt` to src[i] and i the nearest row of `src` to
    tgt[j], ascending in i -> (M, 2) int32 tensor. One read-back (the count)."""
    src, tgt = _feature_rows(src), _feature_rows(tgt)
    L = _lib.lib()
    ns, nt = src.shape[0], tgt.shape[0]
    corr = torch.empty((max(min(ns, nt), 1), 2), dtype=torch.int32, device=src.device)
    ws = _ws_bytes(L.sp_feature_match_mutual_workspace_bytes(ns, nt), src.device)
    count = C.c_uint32(0)
    check(L.sp_feature_match_mutual(_ptr(src), ns, _ptr(tgt), nt, _ptr(corr), C.byref(count), _ptr(ws), ws.numel(), _stream()))
    return corr[:int(count.value)]


def correspondence_points(source_points, target_points, corr):
    """sp_correspondence_points: the matched points (M, 4) of both clouds, in the order of `corr`."""
    s, t = _dev_f32(_points_of(source_points), 4), _dev_f32(_points_of(target_points), 4)
    m = int(corr.shape[0])
    cs = torch.empty((m, 4), dtype=torch.float32, device=s.device)
    ct = torch.empty((m, 4), dtype=torch.float32, device=s.device)
    check(_lib.lib().sp_correspondence_points(_ptr(s), s.shape[0], _ptr(t), t.shape[0], _ptr(corr.contiguous()), m, _ptr(cs), _ptr(ct),
                                              _stream()))
    return cs, ct


def ransac_scores(cs, ct, hypotheses, inlier_distance, min_edge=0.0, edge_ratio=0.9, seed=0):
    """sp_ransac_score: the number of matches each of `hypotheses` triplet poses explains (0 for a triplet that fails a gate) ->
    int32 tensor on the device."""
    cs, ct = _dev_f32(cs, 4), _dev_f32(ct, 4)
    score = torch.empty(max(int(hypotheses), 1), dtype=torch.int32, device=cs.device)
    check(_lib.lib().sp_ransac_score(_ptr(cs), _ptr(ct), cs.shape[0], int(hypotheses), int(seed), inlier_distance, min_edge, edge_ratio,
                                     _ptr(score), _stream()))
    return score[:int(hypotheses)]


def ransac_triplets(seed, hypotheses, m, first=0):
    """sp_ransac_triplets_host: the matches hypotheses first .. first + hypotheses - 1 draw -> (hypotheses, 3) uint32 numpy"""
    out = np.zeros((int(hypotheses), 3), np.uint32)
    check(_lib.lib().sp_ransac_triplets_host(int(seed), int(first), int(hypotheses), int(m), out.ctypes.data_as(C.c_void_p)))
    return out


def ransac_select(scores, cs, ct, guesses, seed=0):
    """sp_ransac_select_host: the `guesses` best hypotheses (ties to the lower index) and their poses in double, from host copies
    of the scores and the matched points (tensors are copied down) -> (poses (B', 4, 4) float64, hypotheses (B',) uint32)."""
    host = lambda a, dt: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dt)  # noqa: E731
    sc, csh, cth = host(scores, np.int32).view(np.uint32), host(cs, np.float32), host(ct, np.float32)
    B = int(guesses)
    poses = np.zeros((max(B, 1), 16), np.float64)
    hyp = np.zeros(max(B, 1), np.uint32)
    count = C.c_size_t(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    check(_lib.lib().sp_ransac_select_host(vp(sc), sc.shape[0], vp(csh), vp(cth), csh.shape[0], int(seed), B, vp(poses), vp(hyp),
                                           C.byref(count)))
    v = int(count.value)
    return poses[:v].reshape(v, 4, 4).transpose(0, 2, 1).copy(), hyp[:v].copy()


@dataclass
class GlobalRegistrationParams:
    """registration::GlobalRegistrationParams (MI355X extension)"""
    hypotheses: int = 50000
    guesses: int = 64
    inlier_distance: float = 1.0   # tau: a match counts for a hypothesis when its residual is below this
    min_edge: float = 0.0          # every source edge of a triplet must be longer
    edge_ratio: float = 0.9        # the shorter of two matching edges against the longer
    seed: int = 0
    method: str = "TRIPLETS"       # or "COMPATIBILITY": the compatibility graph of DESIGN.md 4.22 (min_edge gates its edges too)
    compat_tau: float = 0.1        # two matches are compatible when their two distances differ by less than this
    compat_seeds: int = 64         # consensus sets tried (<= 256)
    compat_k: int = 16             # companions per consensus set (<= 64)


# ------------------------------------------------------------------ compatibility-graph guesses (MI355X extension)
@dataclass
class CompatSeeds:
    """What sp_compat_seeds leaves behind: the seeds in rank order (-1 / 0 beyond the last), optionally every match's degree and
    second-order sum, and the workspace that holds the graph for compat_consensus."""
    m: int
    seed_idx: "torch.Tensor"
    seed_s: "torch.Tensor"
    workspace: "torch.Tensor"
    degree: "torch.Tensor" = None
    s: "torch.Tensor" = None


def compat_seeds(cs, ct, tau=0.1, min_edge=0.0, seeds=64, want_all=False):
    """sp_compat_seeds: the compatibility graph of the matched points cs, ct (M, 4), its second-order row sums on the int8 matrix
    cores, and the `seeds` matches with the largest sums -> CompatSeeds (seed_idx int32, seed_s int32 on the device). want_all:
    also degree and s of every match, (M,) int32. Enqueue only."""
    cs, ct = _dev_f32(cs, 4), _dev_f32(ct, 4)
    L = _lib.lib()
    m, n = int(cs.shape[0]), int(seeds)
    seed_idx = torch.empty(max(n, 1), dtype=torch.int32, device=cs.device)
    seed_s = torch.empty(max(n, 1), dtype=torch.int32, device=cs.device)
    degree = torch.empty(max(m, 1), dtype=torch.int32, device=cs.device) if want_all else None
    s = torch.empty(max(m, 1), dtype=torch.int32, device=cs.device) if want_all else None
    ws = _ws_bytes(L.sp_compat_workspace_bytes(m), cs.device)
    check(L.sp_compat_seeds(_ptr(cs), _ptr(ct), m, tau, min_edge, n, _ptr(seed_idx), _ptr(seed_s), _ptr(degree), _ptr(s), _ptr(ws),
                            ws.numel(), _stream()))
    return CompatSeeds(m, seed_idx[:n], seed_s[:n], ws, None if degree is None else degree[:m], None if s is None else s[:m])


def compat_consensus(graph, k=16, want_s=False):
    """sp_compat_consensus: for every seed of `graph` (a CompatSeeds) its k best companions by second-order compatibility ->
    (seeds, k) int32 on the device, -1 beyond the last; want_s: also their S values. Enqueue only."""
    n, k = int(graph.seed_idx.shape[0]), int(k)
    cons = torch.empty((max(n, 1), max(k, 1)), dtype=torch.int32, device=graph.seed_idx.device)
    cons_s = torch.empty_like(cons) if want_s else None
    check(_lib.lib().sp_compat_consensus(graph.m, _ptr(graph.seed_idx), n, k, _ptr(cons), _ptr(cons_s), _ptr(graph.workspace),
                                         graph.workspace.numel(), _stream()))
    cons = cons.reshape(-1)[:n * k].reshape(n, k)
    return (cons, cons_s.reshape(-1)[:n * k].reshape(n, k)) if want_s else cons


def pose_scores(cs, ct, poses, inlier_distance):
    """sp_pose_score: how many matches each pose explains. poses: (P, 4, 4) row-major matrices (numpy or tensor; uploaded as
    float32) -> int32 tensor (P,) on the device."""
    cs, ct = _dev_f32(cs, 4), _dev_f32(ct, 4)
    P = np.asarray(poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else poses, np.float64).reshape(-1, 4, 4)
    cols = torch.from_numpy(np.ascontiguousarray(P.transpose(0, 2, 1), np.float32).reshape(-1, 16)).to(cs.device)
    score = torch.empty(max(len(P), 1), dtype=torch.int32, device=cs.device)
    check(_lib.lib().sp_pose_score(_ptr(cs), _ptr(ct), cs.shape[0], _ptr(cols), len(P), inlier_distance, _ptr(score), _stream()))
    return score[:len(P)]


def compat_poses(cs, ct, seed_idx, cons):
    """sp_compat_poses_host: the least-squares pose of every consensus set with at least two companions, from host copies of
    everything (tensors are copied down) -> (poses (P, 4, 4) float64, seed ranks (P,) uint32)."""
    host = lambda a, dt: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dt)  # noqa: E731
    csh, cth, si, co = host(cs, np.float32), host(ct, np.float32), host(seed_idx, np.int32), host(cons, np.int32)
    n, k = (co.shape[0], co.shape[1]) if co.ndim == 2 else (0, 0)
    poses = np.zeros((max(n, 1), 16), np.float64)
    rank = np.zeros(max(n, 1), np.uint32)
    count = C.c_size_t(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    check(_lib.lib().sp_compat_poses_host(vp(csh), vp(cth), csh.shape[0], vp(si), vp(co), n, k, vp(poses), vp(rank), C.byref(count)))
    v = int(count.value)
    return poses[:v].reshape(v, 4, 4).transpose(0, 2, 1).copy(), rank[:v].copy()


def compat_select(scores, poses, ranks, guesses):
    """sp_compat_select_host: the `guesses` poses with the highest nonzero score, ties to the earlier seed rank ->
    (poses (B', 4, 4) float64, seed ranks (B',) uint32)."""
    sc = np.ascontiguousarray(scores.detach().cpu().numpy() if isinstance(scores, torch.Tensor) else scores, np.int32).view(np.uint32)
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1, 16)
    rk = np.ascontiguousarray(ranks, np.uint32)
    B = int(guesses)
    out = np.zeros((max(B, 1), 16), np.float64)
    out_rank = np.zeros(max(B, 1), np.uint32)
    count = C.c_size_t(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    check(_lib.lib().sp_compat_select_host(vp(sc), vp(P), vp(rk), len(P), B, vp(out), vp(out_rank), C.byref(count)))
    v = int(count.value)
    return out[:v].reshape(v, 4, 4).transpose(0, 2, 1).copy(), out_rank[:v].copy()


def compat_guesses(cs, ct, params=None):
    """registration::global_guesses with method == COMPATIBILITY on matched points: seeds -> consensus sets -> poses (host,
    double) -> scores -> the params.guesses best -> (poses (B', 4, 4) float64, seed ranks (B',) uint32); empty when no two matches
    are compatible. One read-back for the lists and the points, one for the scores."""
    gp = params or GlobalRegistrationParams(method="COMPATIBILITY")
    none = (np.zeros((0, 4, 4), np.float64), np.zeros(0, np.uint32))
    if cs.shape[0] < 3 or gp.guesses <= 0 or gp.compat_seeds <= 0 or gp.compat_k <= 0:
        return none
    graph = compat_seeds(cs, ct, gp.compat_tau, gp.min_edge, gp.compat_seeds)
    cons = compat_consensus(graph, gp.compat_k)
    poses, ranks = compat_poses(cs, ct, graph.seed_idx, cons)
    if len(poses) == 0:
        return none
    return compat_select(pose_scores(cs, ct, poses, gp.inlier_distance), poses, ranks, gp.guesses)


# ------------------------------------------------------------------ place recognition (MI355X extension)
@dataclass
class ScanContextParams:
    """place_recognition::ScanContextParams (sp_scan_context_params): rings 1..32, sectors even 4..64, max_range finite > 0"""
    rings: int = 20
    sectors: int = 60
    max_range: float = 80.0
    sensor_height: float = 2.0

    def c_struct(self):
        return _lib.ScanContextParams(int(self.rings), int(self.sectors), float(self.max_range), float(self.sensor_height))


@dataclass
class LoopCandidate:
    """One row of ScanContextDatabase.query: the entry's index, its distance in [0, 1], the column shift that attains it and the
    yaw it stands for (shift * 2 pi / sectors: the query is the entry turned by it about z)."""
    index: int
    distance: float
    shift: int
    yaw: float
    sectors: int


def scan_context(cloud, params=None):
    """place_recognition::ScanContext::compute (sp_scan_context_compute): the (rings, sectors) float32 descriptor of a cloud (a
    PointCloudShared or an (N, 4) tensor) on the device. Enqueue only."""
    p = params or ScanContextParams()
    pts = _dev_f32(_points_of(cloud), 4)
    prm = p.c_struct()
    out = torch.empty((max(int(p.rings), 0), max(int(p.sectors), 0)), dtype=torch.float32, device=pts.device)
    check(_lib.lib().sp_scan_context_compute(C.byref(prm), _ptr(pts), pts.shape[0], _ptr(out), _stream()))
    return out


class ScanContextDatabase:
    """place_recognition::ScanContextDatabase (sp_scan_context_db_*): the descriptors of the keyframes so far, searched exactly —
    every entry of the range under every column shift, no pre-filter. add() and search() only enqueue; query() reads back once."""

    def __init__(self, params=None, capacity_hint=0):
        self.params = params or ScanContextParams()
        self._h = C.c_void_p()
        prm = self.params.c_struct()
        check(_lib.lib().sp_scan_context_db_create(C.byref(prm), int(capacity_hint), C.byref(self._h)))
        self._finalizer = weakref.finalize(self, _lib.lib().sp_scan_context_db_destroy, self._h)

    def _descriptor(self, d):
        if isinstance(d, PointCloudShared):
            return scan_context(d, self.params)
        d = _dev_f32(d)
        if tuple(d.shape) != (self.params.rings, self.params.sectors):
            raise SpError(1, f"expected a descriptor of shape ({self.params.rings}, {self.params.sectors}), got {tuple(d.shape)}")
        return d

    def add(self, cloud_or_descriptor):
        """Appends a PointCloudShared's descriptor, or a descriptor from scan_context(); returns the new entry's index."""
        d = self._descriptor(cloud_or_descriptor)
        check(_lib.lib().sp_scan_context_db_add(self._h, _ptr(d), _stream()))
        return self.size() - 1

    def size(self):
        return int(_lib.lib().sp_scan_context_db_size(self._h))

    __len__ = size

    def clear(self):
        check(_lib.lib().sp_scan_context_db_clear(self._h))

    def search(self, descriptor, k, first=0, count=None):
        """sp_scan_context_db_search over the entries [first, first + count): (indices int32, distances float32, shifts int32),
        k rows each on the device, ascending by (distance, index); rows beyond count are -1 / FLT_MAX / 0. Enqueue only."""
        L = _lib.lib()
        d = self._descriptor(descriptor)
        count = self.size() - int(first) if count is None else int(count)
        k = int(k)
        out = torch.empty((3, max(k, 1)), dtype=torch.int32, device=d.device)
        ws = _ws_bytes(L.sp_scan_context_db_search_workspace_bytes(self._h, max(count, 0)), d.device)
        check(L.sp_scan_context_db_search(self._h, _ptr(d), int(first), count, k, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(ws),
                                          ws.numel(), _stream()))
        return out[0, :k], out[1, :k].view(torch.float32), out[2, :k]

    def query(self, descriptor, k, exclude_recent=0):
        """The k nearest entries among all but the `exclude_recent` most recent -> [LoopCandidate], nearest first (fewer than k
        when the range holds fewer). One read-back."""
        count = max(self.size() - int(exclude_recent), 0)
        if count == 0 or k <= 0:
            return []
        idx, dist, shift = self.search(descriptor, k, 0, count)
        rows = torch.stack([idx, dist.view(torch.int32), shift]).cpu().numpy()
        sectors = int(self.params.sectors)
        return [LoopCandidate(int(i), float(np.int32(db).view(np.float32)), int(s), float(np.float32(int(s) * (2.0 * np.pi) / sectors)),
                              sectors)
                for i, db, s in zip(rows[0], rows[1], rows[2]) if i >= 0]


def scan_context_guesses(candidate, steps, sectors=None):
    """place_recognition::initial_guesses (sp_scan_context_guesses_host): `steps` poses Rz(-(shift + delta) 2 pi / sectors), delta
    evenly over [-1/2, 1/2] sector, as 4x4 float32 — the initial guesses Registration.align_batch wants for aligning the query
    to the candidate (a LoopCandidate, or a shift with `sectors`)."""
    shift = candidate.shift if isinstance(candidate, LoopCandidate) else int(candidate)
    sectors = candidate.sectors if isinstance(candidate, LoopCandidate) else int(sectors or ScanContextParams().sectors)
    steps = int(steps)
    prm = ScanContextParams(sectors=sectors).c_struct()
    poses = np.zeros((max(steps, 1), 16), np.float64)
    check(_lib.lib().sp_scan_context_guesses_host(C.byref(prm), shift, steps, poses.ctypes.data_as(C.c_void_p)))
    return [np.ascontiguousarray(T.reshape(4, 4).T, np.float32) for T in poses[:steps]]


# ------------------------------------------------------------------ voxel grid
class VoxelGrid:
    """algorithms/filter/voxel_downsampling.hpp:14-289"""

    def __init__(self, voxel_size):
        if voxel_size <= 0.0:
            raise SpError(1, "voxel_size must be positive")
        self.voxel_size = float(voxel_size)
        self.voxel_size_inv = float(np.float32(1.0) / np.float32(voxel_size))
        self._key_box = None  # the remembered key box is in units of the old voxel size  # voxel_downsampling.hpp:27
        self.min_voxel_count = 1

    def set_voxel_size(self, voxel_size):
        if voxel_size <= 0.0:
            raise SpError(1, "voxel_size must be positive")
        self.voxel_size = float(voxel_size)
        self.voxel_size_inv = float(np.float32(1.0) / np.float32(voxel_size))

    def get_voxel_size(self):
        return self.voxel_size

    def set_min_voxel_count(self, n):
        self.min_voxel_count = int(n)

    def compute_voxel_bit(self, points):
        p = _dev_f32(_points_of(points), 4)
        keys = torch.empty(p.shape[0], dtype=torch.int64, device=p.device)  # bit pattern of the uint64 keys
        check(_lib.lib().sp_voxel_keys(_ptr(p), p.shape[0], self.voxel_size_inv, _ptr(keys), _stream()))
        return keys

    def downsampling(self, cloud, return_keys=False, boxed=True):
        """downsampling(cloud, result) (voxel_downsampling.hpp:64-79). Synchronises to read the voxel count, as the
        reference's host aggregation does. boxed=True sorts keys compressed to the (widened) bounding box of the PREVIOUS
        cloud's voxel coordinates — scans of one sensor have similar extents — verifies on the device that the cloud fits,
        and falls back to the 64-bit sort when it does not: identical results either way."""
        L = _lib.lib()
        return _boxed_downsampling(self, cloud, return_keys, boxed,
                                   lambda p, n, box6: L.sp_voxel_key_box(p, n, self.voxel_size_inv, box6, _stream()),
                                   lambda p, n, rest: L.sp_voxel_downsample_report(p, n, self.voxel_size_inv, self.min_voxel_count,
                                                                                   *rest))


def _boxed_downsampling(grid, cloud, return_keys, boxed, key_box, report):
    """VoxelGrid / PolarGrid.downsampling over sp_voxel_downsample_report / sp_polar_downsample_report. key_box(points, n, box6)
    and report(points, n, rest) call the C entry points with the grid's own key arguments; grid._key_box is the remembered box."""
    pc = cloud if isinstance(cloud, PointCloudShared) else PointCloudShared(cloud)
    p = _dev_f32(pc.points, 4)
    n = p.shape[0]
    out = PointCloudShared(device=p.device)
    if n == 0:
        return (out, torch.empty(0, dtype=torch.int64, device=p.device)) if return_keys else out
    L = _lib.lib()
    nbytes = L.sp_voxel_downsample_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    o_p = torch.empty((n, 4), dtype=torch.float32, device=p.device)
    rgb = pc.rgb if pc.has_rgb() else None
    inten = pc.intensities if pc.has_intensity() else None
    ts = pc.timestamp_offsets if pc.has_timestamps() else None
    o_c = torch.empty((n, 4), dtype=torch.float32, device=p.device) if rgb is not None else None
    o_i = torch.empty(n, dtype=torch.float32, device=p.device) if inten is not None else None
    o_t = torch.empty(n, dtype=torch.float32, device=p.device) if ts is not None else None
    o_k = torch.empty(n, dtype=torch.int64, device=p.device) if return_keys else None
    # One read-back at the end: voxel count, boxed-path status, and this cloud's key box (sharded, found by the key
    # kernel on the way), which the NEXT call uses, widened by a margin, to sort keys compressed to that box. A cloud that
    # leaves the remembered box is detected (status != 0) and redone with its own exact box, so results never depend on
    # the guess. The first call of a grid has no guess: it computes the box first (the key-box call, one small
    # read-back) — every call sorts compressed keys; the 64-bit sort is left for boxes of >= 2^32 cells.
    # (the report call: all of it in ONE 8-word record the call's last kernel stores — no status word and sharded
    # box to initialise and fold)
    info = torch.zeros(16, dtype=torch.int32, device=p.device)
    base = info.data_ptr()
    args = (_ptr(rgb), _ptr(inten), _ptr(ts), _ptr(o_p), _ptr(o_c), _ptr(o_i), _ptr(o_t), _ptr(o_k), None)

    def run(box):
        check(report(_ptr(p), n, args + (None if box is None else box.ctypes.data_as(C.c_void_p), C.c_void_p(base), _ptr(ws),
                                         nbytes, _stream())))
        c = info.cpu().numpy()
        return c, c[2:8].astype(np.int64)

    guess = getattr(grid, "_key_box", None) if boxed else None
    if guess is None and boxed:
        check(key_box(_ptr(p), n, C.c_void_p(base + 32)))
        b0 = info[8:14].cpu().numpy().astype(np.int64)
        guess = np.ascontiguousarray(b0.astype(np.int32)) if (b0[:3] <= b0[3:]).all() else None
    counts, box = run(guess)
    if counts[1] != 0:  # the cloud left the remembered box: again, with its own
        counts, box = run(np.ascontiguousarray(box.astype(np.int32)))
    if boxed and (box[:3] <= box[3:]).all():
        margin = np.maximum(2, (box[3:] - box[:3] + 1) // 8)
        lo = np.maximum(box[:3] - margin, 0)
        hi = np.minimum(box[3:] + margin, (1 << 21) - 1)
        # Keep what earlier clouds needed as well (one grid usually serves several scans in turn — source and target
        # of a registration —, and a guess that forgets the other scan is redone every call), unless that has grown to
        # more than 8x the cells this cloud needs.
        prev = getattr(grid, "_key_box", None)
        if prev is not None:
            ulo, uhi = np.minimum(lo, prev[:3]), np.maximum(hi, prev[3:])
            if np.prod((uhi - ulo + 1).astype(np.float64)) <= 8.0 * np.prod((hi - lo + 1).astype(np.float64)):
                lo, hi = ulo, uhi
        grid._key_box = np.ascontiguousarray(np.concatenate([lo, hi]).astype(np.int32))
    v = int(counts[0])
    out.points = o_p[:v]
    out.rgb = None if o_c is None else o_c[:v]
    out.intensities = None if o_i is None else o_i[:v]
    out.timestamp_offsets = None if o_t is None else o_t[:v]
    return (out, o_k[:v]) if return_keys else out


# ------------------------------------------------------------------ polar grid
COORDINATE_SYSTEMS = ("LIDAR", "CAMERA")  # algorithms/common/coordinate_system.hpp:11


def coordinate_system_from_string(s):
    """coordinate_system.hpp:13-24: "lidar" / "camera" in any case; anything else raises."""
    u = str(s).upper()
    if u not in _lib.COORD:
        raise SpError(1, f"Invalid coordinate system: {s}")
    return u


class PolarGrid:
    """algorithms/filter/polar_downsampling.hpp:104-452: VoxelGrid's device path with the polar key (distance, elevation,
    azimuth). coord: "LIDAR" (default) or "CAMERA"; the angle sizes are in radians."""

    def __init__(self, distance_voxel_size, elevation_voxel_size, azimuth_voxel_size, coord="LIDAR"):
        if distance_voxel_size <= 0.0 or elevation_voxel_size <= 0.0 or azimuth_voxel_size <= 0.0:
            raise SpError(1, "voxel sizes must be positive")
        self.coord = coordinate_system_from_string(coord)
        self.set_distance_voxel_size(distance_voxel_size)
        self.set_elevation_voxel_size(elevation_voxel_size)
        self.set_azimuth_voxel_size(azimuth_voxel_size)
        self.min_voxel_count = 1

    def _size(self, name, v):
        if v <= 0.0:
            raise SpError(1, f"{name}_voxel_size must be positive")
        setattr(self, f"{name}_voxel_size", float(v))
        setattr(self, f"{name}_voxel_size_inv", float(np.float32(1.0) / np.float32(v)))
        self._key_box = None  # the remembered key box is in units of the old size

    def set_distance_voxel_size(self, v): self._size("distance", v)  # noqa: E704
    def get_distance_voxel_size(self): return self.distance_voxel_size  # noqa: E704
    def set_elevation_voxel_size(self, v): self._size("elevation", v)  # noqa: E704
    def get_elevation_voxel_size(self): return self.elevation_voxel_size  # noqa: E704
    def set_azimuth_voxel_size(self, v): self._size("azimuth", v)  # noqa: E704
    def get_azimuth_voxel_size(self): return self.azimuth_voxel_size  # noqa: E704

    def set_min_voxel_count(self, n):
        self.min_voxel_count = int(n)

    def get_min_voxel_count(self):
        return self.min_voxel_count

    def set_coordinate_system(self, coord):
        self.coord = coordinate_system_from_string(coord)
        self._key_box = None

    def get_coordinate_system(self):
        return self.coord

    def _key_args(self):
        return (_lib.COORD[self.coord], self.distance_voxel_size_inv, self.elevation_voxel_size_inv, self.azimuth_voxel_size_inv)

    def compute_polar_bit(self, points):
        """kernel::compute_polar_bit (polar_downsampling.hpp:30-100) of every point, on the device: int64 tensor holding the
        bit patterns of the uint64 keys (~0: invalid)."""
        p = _dev_f32(_points_of(points), 4)
        keys = torch.empty(p.shape[0], dtype=torch.int64, device=p.device)
        check(_lib.lib().sp_polar_keys(_ptr(p), p.shape[0], *self._key_args(), _ptr(keys), _stream()))
        return keys

    def downsampling(self, cloud, return_keys=False, boxed=True):
        """downsampling(cloud, result) (polar_downsampling.hpp:200-236), with VoxelGrid.downsampling's calling shape and
        protocol (keys compressed to the remembered box of the previous clouds' polar fields; a redo when a cloud leaves it)."""
        L = _lib.lib()
        k = self._key_args()
        return _boxed_downsampling(self, cloud, return_keys, boxed,
                                   lambda p, n, box6: L.sp_polar_key_box(p, n, *k, box6, _stream()),
                                   lambda p, n, rest: L.sp_polar_downsample_report(p, n, *k, self.min_voxel_count, *rest))


# ------------------------------------------------------------------ transform / filters
def transform_points(points, T):
    p = _dev_f32(points, 4)
    out = torch.empty_like(p)
    a = _T16(T)
    check(_lib.lib().sp_transform(_ptr(p), None, None, p.shape[0], a.ctypes.data_as(C.c_void_p), _ptr(out), None, None,
                                  _stream()))
    return out


def transform(cloud, T):
    """transform::transform (common/transform.hpp:45-101), in place on the cloud's attributes."""
    a = _T16(T)
    n = cloud.size()
    covs = cloud.covs if cloud.has_cov() else None
    nrm = cloud.normals if cloud.has_normal() else None
    check(_lib.lib().sp_transform(_ptr(cloud.points), _ptr(covs), _ptr(nrm), n, a.ctypes.data_as(C.c_void_p),
                                  _ptr(cloud.points), _ptr(covs), _ptr(nrm), _stream()))
    return cloud


def transform_copy(cloud, T):
    out = PointCloudShared(cloud.points.clone(), None if cloud.covs is None else cloud.covs.clone(),
                           None if cloud.normals is None else cloud.normals.clone(), cloud.rgb, cloud.intensities,
                           cloud.timestamp_offsets, device=cloud.points.device)
    return transform(out, T)


def relative_twist(previous_pose, current_pose):
    """se3_log(previous_pose^-1 * current_pose) as the deskew takes it (sp_relative_twist_host): 6 floats, rotation first."""
    tw = np.zeros(6, np.float32)
    a, b = _T16(previous_pose), _T16(current_pose)
    _lib.lib().sp_relative_twist_host(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), tw.ctypes.data_as(C.c_void_p))
    return tw


def _deskew_buffers(cloud):
    """What both deskews hand their kernel: (points, stamps, covs or None, normals or None, out). `out` has fresh points,
    covariances and normals, shares the cloud's rgb, intensities and stamps, and carries its start / end time where it has them."""
    p = _dev_f32(cloud.points, 4)
    ts = _dev_f32(cloud.timestamp_offsets)
    covs = _dev_f32(cloud.covs, 16) if cloud.has_cov() else None
    nrm = _dev_f32(cloud.normals, 4) if cloud.has_normal() else None
    out = PointCloudShared(torch.empty_like(p), None if covs is None else torch.empty_like(covs),
                           None if nrm is None else torch.empty_like(nrm), cloud.rgb, cloud.intensities, cloud.timestamp_offsets,
                           device=p.device)
    for k in ("start_time_ms", "end_time_ms"):
        if hasattr(cloud, k):
            setattr(out, k, getattr(cloud, k))
    return p, ts, covs, nrm, out


def deskew_point_cloud_constant_velocity(cloud, previous_pose, current_pose, inter_scan_duration_seconds=-1.0):
    """deskew::deskew_point_cloud_constant_velocity (deskew/relative_pose_deskew.hpp:36-178): a new cloud with every point moved
    from the sensor frame at its time stamp (timestamp_offsets, ms) into the frame of `current_pose`, assuming constant body
    velocity from `previous_pose`; normals and covariances are rotated with it, the other attributes are shared. None where the
    reference returns false: an empty cloud, no time stamps, or no positive duration (the fallback is the cloud's own
    (end_time_ms - start_time_ms) * 1e-3 when it carries those attributes)."""
    n = cloud.size()
    if n == 0 or not cloud.has_timestamps():
        return None
    duration = np.float32(inter_scan_duration_seconds)
    if not duration > 0.0:
        duration = np.float32((float(getattr(cloud, "end_time_ms", 0.0)) - float(getattr(cloud, "start_time_ms", 0.0))) * 1e-3)
    if not duration > 0.0:
        return None
    p, ts, covs, nrm, out = _deskew_buffers(cloud)
    tw = relative_twist(previous_pose, current_pose)
    check(_lib.lib().sp_deskew_constant_velocity(_ptr(p), _ptr(covs), _ptr(nrm), _ptr(ts), n, tw.ctypes.data_as(C.c_void_p),
                                                 float(duration), _ptr(out.points), _ptr(out.covs), _ptr(out.normals), _stream()))
    return out


# ------------------------------------------------------------------ IMU preintegration / IMU deskew
@dataclass
class IMUPreintegrationParams:
    """imu::IMUPreintegrationParams (algorithms/imu/imu_preintegration.hpp:138-166)"""
    gravity: tuple = (0.0, 0.0, -9.80665)
    accel_scale: float = 1.0
    gyro_noise_density: float = 0.0
    accel_noise_density: float = 0.0
    gyro_bias_rw_density: float = 0.0
    accel_bias_rw_density: float = 0.0

    def _c(self):
        return _lib.ImuParams((C.c_float * 3)(*[float(g) for g in self.gravity]), self.accel_scale, self.gyro_noise_density,
                              self.accel_noise_density, self.gyro_bias_rw_density, self.accel_bias_rw_density)


class IMUDeskewStatus(enum.IntEnum):
    """deskew::IMUDeskewStatus (algorithms/deskew/imu_deskew.hpp:32-38)"""
    success = 0
    insufficient_imu_coverage = 1
    no_timestamps = 2
    invalid_scan_duration = 3
    empty_cloud = 4


@dataclass
class PreintegrationResult:
    """imu::PreintegrationResult with its Jacobians (imu_preintegration.hpp:98-135), numpy arrays in the usual row-major view"""
    Delta_R: np.ndarray
    Delta_v: np.ndarray
    Delta_p: np.ndarray
    dt_total: float
    J_R_bg: np.ndarray
    J_v_bg: np.ndarray
    J_v_ba: np.ndarray
    J_p_bg: np.ndarray
    J_p_ba: np.ndarray
    covariance: np.ndarray


def _f32(a, n):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1))
    if a.size != n:
        raise SpError(1, f"expected {n} values, got {a.size}")
    return a


def _bias6(bias):
    return np.zeros(6, np.float32) if bias is None else _f32(bias, 6)


def _hp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class IMUPreintegration:
    """imu::IMUPreintegration (imu_preintegration.hpp:180-529): the C library's host integrator (sp_imu_preint_*), so the
    arithmetic exists once. A bias is six values, (gyro_bias, accel_bias); matrices are row-major numpy arrays."""

    def __init__(self, params=None):
        self.params = params or IMUPreintegrationParams()
        self._h = C.c_void_p()
        check(_lib.lib().sp_imu_preint_create(C.byref(self.params._c()), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.lib().sp_imu_preint_destroy(self._h)
            self._h = None

    def reset(self, bias=None, initial_covariance=None, R_world_body=None):
        cov = None if initial_covariance is None else _f32(np.asarray(initial_covariance, np.float32).T, 225)
        R = None if R_world_body is None else _f32(np.asarray(R_world_body, np.float32).T, 9)
        check(_lib.lib().sp_imu_preint_reset(self._h, _hp(_bias6(bias)), _hp(cov), _hp(R)))

    def integrate(self, timestamp, gyro, accel):
        check(_lib.lib().sp_imu_preint_integrate(self._h, float(timestamp), _hp(_f32(gyro, 3)), _hp(_f32(accel, 3))))

    def integrate_batch(self, stamps, gyro, accel):
        for t, g, a in zip(stamps, gyro, accel):
            self.integrate(t, g, a)

    def _get(self, bias):
        st = _lib.ImuState()
        check(_lib.lib().sp_imu_preint_get(self._h, None if bias is None else _hp(_bias6(bias)), C.byref(st)))
        m3 = lambda f: np.array(f, np.float32).reshape(3, 3).T.copy()  # noqa: E731  (column-major at the C ABI)
        return PreintegrationResult(m3(st.Delta_R), np.array(st.Delta_v, np.float32), np.array(st.Delta_p, np.float32),
                                    float(st.dt_total), m3(st.J_R_bg), m3(st.J_v_bg), m3(st.J_v_ba), m3(st.J_p_bg), m3(st.J_p_ba),
                                    np.array(st.covariance, np.float32).reshape(15, 15).T.copy())

    def get_raw(self):
        return self._get(None)

    def get_corrected(self, new_bias):
        return self._get(_bias6(new_bias))

    def predict_relative_transform(self, R_world_body_i, v_world_i, current_bias=None):
        T = np.zeros(16, np.float32)
        check(_lib.lib().sp_imu_preint_predict_relative(self._h, _hp(_f32(np.asarray(R_world_body_i, np.float32).T, 9)),
                                                        _hp(_f32(v_world_i, 3)), _hp(_bias6(current_bias)), _hp(T)))
        return T.reshape(4, 4).T.copy()

    def predict_transform(self, T_world_body_i, v_world_i, current_bias=None):
        T = np.zeros(16, np.float32)
        check(_lib.lib().sp_imu_preint_predict_transform(self._h, _hp(_f32(_T16(T_world_body_i), 16)), _hp(_f32(v_world_i, 3)),
                                                         _hp(_bias6(current_bias)), _hp(T)))
        return T.reshape(4, 4).T.copy()

    def get_dt_total(self):
        return self.get_raw().dt_total

    def has_measurements(self):
        return _lib.lib().sp_imu_preint_num_measurements(self._h) > 0

    def get_params(self):
        return self.params


def interpolate_measurement(before, after, timestamp):
    """imu::interpolate_measurement (imu_preintegration.hpp:32-42); a measurement is (timestamp, gyro[3], accel[3])."""
    span = after[0] - before[0]
    if span <= 0.0:
        return before
    alpha = min(max((timestamp - before[0]) / span, 0.0), 1.0)
    mix = lambda a, b: ((1.0 - alpha) * np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
                        + alpha * np.asarray(b, np.float32).astype(np.float64)).astype(np.float32)
    return (timestamp, mix(before[1], after[1]), mix(before[2], after[2]))


def build_measurement_window(measurements, start_timestamp, end_timestamp):
    """imu::build_measurement_window (imu_preintegration.hpp:55-87): the samples of (start, end] with one interpolated at
    either boundary when bracketing samples exist."""
    window = []
    if end_timestamp <= start_timestamp:
        return window
    before_start = None
    for m in measurements:
        if m[0] <= start_timestamp:
            before_start = m
            continue
        if m[0] > end_timestamp:
            if not window and before_start is not None:
                window.append(interpolate_measurement(before_start, m, start_timestamp))
            if window and window[-1][0] < end_timestamp:
                window.append(interpolate_measurement(window[-1], m, end_timestamp))
            break
        if not window and before_start is not None:
            window.append(interpolate_measurement(before_start, m, start_timestamp) if before_start[0] < start_timestamp
                          else before_start)
        window.append(m)
    return window


def imu_deskew_trajectory(stamps, gyro, accel, scan_start_sec, scan_duration_sec, T_imu_to_lidar, bias=None, params=None,
                          R_world_body=None, v_world=None, gyro_only=False):
    """Steps 1-3 of deskew::deskew_point_cloud_imu (deskew/imu_deskew.hpp:158-285) on the host (sp_imu_deskew_trajectory_host):
    (trajectory, status), the trajectory an (m, 8) float32 array of q xyzw, t xyz, seconds from scan start, or None."""
    stamps = np.ascontiguousarray(np.asarray(stamps, np.float64).reshape(-1))
    n = stamps.size
    ga = np.ascontiguousarray(np.concatenate([np.asarray(gyro, np.float32).reshape(n, 3), np.asarray(accel, np.float32).reshape(n, 3)],
                                             axis=1))
    traj = np.zeros((n + 1, 8), np.float32)
    m, status = C.c_size_t(0), C.c_int(0)
    R = np.eye(3, dtype=np.float32) if R_world_body is None else np.asarray(R_world_body, np.float32)
    v = np.zeros(3, np.float32) if v_world is None else v_world
    check(_lib.lib().sp_imu_deskew_trajectory_host(_hp(stamps), _hp(ga), n, float(scan_start_sec), float(scan_duration_sec),
                                                   _hp(_f32(_T16(T_imu_to_lidar), 16)), _hp(_bias6(bias)),
                                                   C.byref((params or IMUPreintegrationParams())._c()), _hp(_f32(R.T, 9)),
                                                   _hp(_f32(v, 3)), int(bool(gyro_only)), _hp(traj), n + 1, C.byref(m),
                                                   C.byref(status)))
    status = IMUDeskewStatus(status.value)
    return (traj[:m.value].copy() if status == IMUDeskewStatus.success else None), status


def imu_deskew_intervals(trajectory):
    """The (m - 1, 16) interval rows sp_deskew_imu reads (sp_imu_deskew_intervals_host)."""
    traj = np.ascontiguousarray(trajectory, np.float32)
    rows = np.zeros((traj.shape[0] - 1, 16), np.float32)
    check(_lib.lib().sp_imu_deskew_intervals_host(_hp(traj), traj.shape[0], _hp(rows)))
    return rows


def deskew_point_cloud_imu(cloud, stamps, gyro, accel, scan_start_sec, T_imu_to_lidar, bias=None, params=None, R_world_body=None,
                           v_world=None, gyro_only=False):
    """deskew::deskew_point_cloud_imu (deskew/imu_deskew.hpp:122-417): (a new cloud, status) with every point moved from the
    sensor frame at its time stamp (timestamp_offsets, ms) into the frame at scan start along the trajectory the IMU samples give;
    normals and covariances are rotated with it, the other attributes are shared. The scan lasts
    (end_time_ms - start_time_ms) * 1e-3 seconds, both attributes of the cloud. (None, status) where the reference returns false."""
    n = cloud.size()
    if n == 0:
        return None, IMUDeskewStatus.empty_cloud
    if not cloud.has_timestamps():
        return None, IMUDeskewStatus.no_timestamps
    duration = (float(getattr(cloud, "end_time_ms", 0.0)) - float(getattr(cloud, "start_time_ms", 0.0))) * 1e-3
    traj, status = imu_deskew_trajectory(stamps, gyro, accel, scan_start_sec, duration, T_imu_to_lidar, bias, params, R_world_body,
                                         v_world, gyro_only)
    if traj is None:
        return None, status
    p, ts, covs, nrm, out = _deskew_buffers(cloud)
    rows = torch.from_numpy(imu_deskew_intervals(traj)).to(p.device)  # a pageable copy: stream-ordered, returns when it is staged
    check(_lib.lib().sp_deskew_imu(_ptr(p), _ptr(covs), _ptr(nrm), _ptr(ts), n, _ptr(rows), rows.shape[0], _ptr(out.points),
                                   _ptr(out.covs), _ptr(out.normals), _stream()))
    return out, status


def box_filter_flags(points, min_distance, max_distance):
    p = _dev_f32(_points_of(points), 4)
    flags = torch.empty(p.shape[0], dtype=torch.uint8, device=p.device)
    check(_lib.lib().sp_box_filter_flags(_ptr(p), p.shape[0], min_distance, max_distance, _ptr(flags), _stream()))
    return flags


def compact_by_flags(rows, flags, want_indices=False):
    """FilterByFlags::filter_by_flags / calculate_indices (common/filter_by_flags.hpp:30-99) on the device."""
    L = _lib.lib()
    n = rows.shape[0]
    row_bytes = rows.element_size() * (rows.numel() // max(n, 1)) if n else 4
    out = torch.empty_like(rows)
    idx = torch.empty(n, dtype=torch.int32, device=rows.device) if want_indices else None
    n_out = torch.zeros(1, dtype=torch.int32, device=rows.device)
    nbytes = L.sp_compact_workspace_bytes(n)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=rows.device)
    check(L.sp_compact_by_flags(_ptr(rows), n, row_bytes, _ptr(flags), _ptr(out), _ptr(idx), _ptr(n_out), _ptr(ws),
                                nbytes, _stream()))
    v = int(n_out.item())
    return (out[:v], idx) if want_indices else out[:v]


def _normals_or_covs(cloud):
    nrm = _dev_f32(cloud.normals, 4) if cloud.has_normal() else None
    covs = _dev_f32(cloud.covs, 16) if cloud.has_cov() else None
    return nrm, covs


def _compact_cloud_by_flags(cloud, flags, want_indices):
    """Every attribute a (non-empty) cloud carries through one sp_compact_by_flags_multi: the new tensors by name, the count and,
    if wanted, every point's new index (-1: removed). One count is read back."""
    L = _lib.lib()
    n = cloud.size()
    names = [k for k in _CLOUD_ATTRS if (t := getattr(cloud, k)) is not None and t.shape[0] == n]
    src = [getattr(cloud, k) for k in names]
    for t in src:
        if not (t.is_cuda and t.is_contiguous()):
            raise SpError(1, "expected contiguous CUDA tensors")
    dst = [torch.empty_like(t) for t in src]
    na = len(src)
    rows = (C.c_void_p * na)(*[t.data_ptr() for t in src])
    rows_out = (C.c_void_p * na)(*[t.data_ptr() for t in dst])
    row_bytes = (C.c_size_t * na)(*[t.element_size() * (t.numel() // n) for t in src])
    dev = cloud.points.device
    idx = torch.empty(n, dtype=torch.int32, device=dev) if want_indices else None
    n_out = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = L.sp_compact_workspace_bytes(n)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    check(L.sp_compact_by_flags_multi(rows, row_bytes, rows_out, na, n, _ptr(flags), _ptr(idx), _ptr(n_out), _ptr(ws), nbytes,
                                      _stream()))
    m = int(n_out.item())
    return {k: t[:m] for k, t in zip(names, dst)}, m, idx


def angle_incidence_filter(cloud, min_angle, max_angle, return_flags=False):
    """PreprocessFilter::angle_incidence_filter (filter/preprocess_filter.hpp:147-160, preprocess_operator/
    angle_incidence_filter_operator.hpp:23-110): a new cloud with the points whose angle of incidence (between the ray from the
    origin and the normal, sign ignored) lies in [min_angle, max_angle]; the normal is the cloud's, or extract_normal of its
    covariance. Every attribute is compacted by the same flags (sp_angle_incidence_flags, then sp_compact_by_flags_multi on the
    same stream, one count read back). An empty cloud comes back as it is, before any check."""
    n = cloud.size()
    if n == 0:
        return (cloud, None) if return_flags else cloud
    L = _lib.lib()
    p = _dev_f32(cloud.points, 4)
    nrm, covs = _normals_or_covs(cloud)
    flags = torch.empty(n, dtype=torch.uint8, device=p.device)
    check(L.sp_angle_incidence_flags(_ptr(p), _ptr(nrm), _ptr(covs), n, min_angle, max_angle, _ptr(flags), _stream()))
    moved, _, _ = _compact_cloud_by_flags(cloud, flags, False)
    out = PointCloudShared(device=p.device, **moved)
    for k in ("start_time_ms", "end_time_ms"):
        if hasattr(cloud, k):
            setattr(out, k, getattr(cloud, k))
    return (out, flags) if return_flags else out


def correct_intensity(cloud, exponent=2.0, scale=1.0, min_intensity=0.0, max_intensity=1000.0, ref_distance=1.0, angle_exponent=0.0):
    """intensity_correction::correct_intensity (filter/intensity_correction.hpp:50-135): cloud.intensities in place,
    I' = clamp(I * (|p| / ref_distance)^exponent * angle_factor * scale, min, max); the angle factor needs normals or covariances
    and a non-zero angle_exponent. The reference's checks in its order; an empty cloud returns before them."""
    n = cloud.size()
    if n == 0:
        return
    nrm, covs = _normals_or_covs(cloud)
    inten = _dev_f32(cloud.intensities) if cloud.has_intensity() else None
    check(_lib.lib().sp_intensity_correct(_ptr(_dev_f32(cloud.points, 4)), _ptr(nrm), _ptr(covs), _ptr(inten), n, exponent, scale,
                                          min_intensity, max_intensity, ref_distance, angle_exponent, _stream()))


def _intensity_gaussian(cloud, neighbors, sigma_azimuth, sigma_elevation, sigma_range, mean_min, k_limit):
    n = cloud.size()
    if n == 0:
        return
    idx = neighbors.indices if isinstance(neighbors, KNNResult) else neighbors
    k = int(idx.shape[1]) if idx.dim() == 2 else 0
    if idx.dtype != torch.int32 or not idx.is_contiguous() or (k and idx.shape[0] != n):
        raise SpError(1, "expected a contiguous int32 (N, k) tensor of neighbour indices")
    k_use = k_limit if 0 < k_limit < k else k
    inten = _dev_f32(cloud.intensities) if cloud.has_intensity() else None
    out = None if inten is None else torch.empty_like(inten)
    check(_lib.lib().sp_intensity_gaussian(_ptr(_dev_f32(cloud.points, 4)), _ptr(inten), _ptr(idx), n, k, k_use, sigma_azimuth,
                                           sigma_elevation, sigma_range, mean_min, _ptr(out), _stream()))
    cloud.intensities = out  # (the reference swaps a fresh vector in)


def smooth_intensity(cloud, neighbors, sigma_azimuth, sigma_elevation, sigma_range=0.05, k_limit=0):
    """intensity_gaussian::smooth_intensity (filter/intensity_gaussian.hpp:88-151): cloud.intensities replaced by their
    directional Gaussian mean over the first k_limit (0: all) neighbours of `neighbors` (a KNNResult of the cloud on itself)."""
    _intensity_gaussian(cloud, neighbors, sigma_azimuth, sigma_elevation, sigma_range, 0.0, k_limit)


def normalize_intensity_local_mean(cloud, neighbors, sigma_azimuth, sigma_elevation, sigma_range=0.05, mean_min=1e-3, k_limit=0):
    """intensity_local_mean_norm::normalize (filter/intensity_local_mean_norm.hpp:36-113): I / max(local mean, mean_min)."""
    if cloud.size() and mean_min <= 0.0:  # (:72-74: the last of the reference's checks; the library reports the ones before it)
        k = neighbors.k if isinstance(neighbors, KNNResult) else (neighbors.shape[1] if neighbors.dim() == 2 else 0)
        if cloud.has_intensity() and k >= 1 and min(sigma_azimuth, sigma_elevation, sigma_range) > 0.0:
            raise SpError(2, "[intensity_local_mean_norm::normalize] mean_min must be positive")
        mean_min = 1.0  # (selects the normalisation's texts)
    _intensity_gaussian(cloud, neighbors, sigma_azimuth, sigma_elevation, sigma_range, mean_min, k_limit)


def intensity_zscore(cloud, neighbors, sigma_min=0.01):
    """intensity_zscore::compute (filter/intensity_zscore.hpp:40-72): cloud.intensities replaced by (I - local mean) / local sigma
    over the neighbours of `neighbors` (a KNNResult of the cloud on itself, or its index tensor), 0 where sigma < sigma_min. The
    reference's checks in its order (sp_intensity_zscore reports them); an empty cloud returns before them."""
    n = cloud.size()
    if n == 0:
        return
    idx = neighbors.indices if isinstance(neighbors, KNNResult) else neighbors
    k = int(idx.shape[1]) if idx is not None and idx.dim() == 2 else 0
    if k and (idx.dtype != torch.int32 or not idx.is_contiguous() or idx.shape[0] != n):
        raise SpError(1, "expected a contiguous int32 (N, k) tensor of neighbour indices")
    inten = _dev_f32(cloud.intensities) if cloud.has_intensity() else None
    out = None if inten is None else torch.empty_like(inten)
    check(_lib.lib().sp_intensity_zscore(_ptr(inten), _ptr(idx) if k else None, n, k, k, sigma_min, _ptr(out), _stream()))
    cloud.intensities = out  # (the reference swaps a fresh vector in)


class OutlierRemoval:
    """filter::OutlierRemoval (filter/outlier_removal_filter.hpp:13-242). statistical() and radius() filter `cloud` in place:
    the kNN search is the caller's KDTree as it is, the flags come from sp_outlier_statistical_flags / sp_outlier_radius_flags on
    the same stream (the reference waits after each of its kernels), and every attribute goes through one
    sp_compact_by_flags_multi, which also leaves the indices calculate_indices() returns. Kept from the reference: the SQUARED
    neighbour distances are averaged and compared as they are, radius() compares the squared distance with `radius` itself
    (:178-188), and too few points print its message and leave the cloud untouched."""

    def __init__(self):
        self.neighbors = KNNResult()
        self.flags = None
        self.indices = None
        self.local_mean_distance = None
        self.statistics = None  # device tensor: global mean, variance, threshold, n

    def statistical(self, cloud, tree, mean_k, stddev_mul_thresh, remove_from_tree=False):
        n = cloud.size()
        if n < mean_k:
            print(f"Not enough points in the cloud [ points = {n}, mean_k = {mean_k} ]", file=sys.stderr)
            return
        if n == 0:
            return
        L = _lib.lib()
        tree.knn_search_async(cloud, mean_k, self.neighbors)
        dev = cloud.points.device
        self.flags = torch.empty(n, dtype=torch.uint8, device=dev)
        self.local_mean_distance = torch.empty(n, dtype=torch.float32, device=dev)
        self.statistics = torch.empty(4, dtype=torch.float32, device=dev)
        nbytes = L.sp_outlier_workspace_bytes(n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(L.sp_outlier_statistical_flags(_ptr(self.neighbors.distances), n, mean_k, mean_k, stddev_mul_thresh, _ptr(self.flags),
                                             _ptr(self.local_mean_distance), _ptr(self.statistics), _ptr(ws), nbytes, _stream()))
        self._filter_by_flags(cloud)
        if remove_from_tree:
            tree.remove_nodes_by_flags(self.get_flags(), self.calculate_indices())

    def radius(self, cloud, tree, min_k, radius, remove_from_tree=False):
        n = cloud.size()
        if n < min_k:
            print(f"Not enough points in the cloud [ points = {n}, min_k = {min_k} ]", file=sys.stderr)
            return
        if n == 0:
            return
        tree.knn_search_async(cloud, min_k + 1, self.neighbors)  # (the tree holds the point itself: :162-163)
        self.flags = torch.empty(n, dtype=torch.uint8, device=cloud.points.device)
        check(_lib.lib().sp_outlier_radius_flags(_ptr(self.neighbors.distances), n, min_k + 1, min_k, radius, _ptr(self.flags),
                                                 _stream()))
        self._filter_by_flags(cloud)
        if remove_from_tree:
            tree.remove_nodes_by_flags(self.get_flags(), self.calculate_indices())

    def get_flags(self):
        """1 for the points of the last call that stayed, 0 for the removed ones"""
        return self.flags

    def calculate_indices(self):
        """the new index of every point of the last call, -1 for a removed one (left by the compaction)"""
        return self.indices

    def _filter_by_flags(self, cloud):
        moved, _, self.indices = _compact_cloud_by_flags(cloud, self.flags, True)
        for k, t in moved.items():  # (the attributes the cloud lacks stay as they are)
            setattr(cloud, k, t)


@dataclass
class FpsResult:
    order: torch.Tensor   # int32 [S]: the i-th selected index, repeats included
    flags: torch.Tensor   # uint8 [N]: 1 selected, 0 not
    min_d2: torch.Tensor  # float32 [N]: each point's squared distance to the nearest selected point (before the last selection)


def farthest_point_sampling(points, sampling_num, first_index, form=None):
    """FarthestPointSamplingOperator::apply's chain of argmax decisions (filter/preprocess_operator/
    farthest_point_sampling_operator.hpp:27-91) on the device, from `first_index` (the reference draws it from the operator's
    own std::mt19937: PreprocessFilter.farthest_point_sampling in the C++ facade does that draw). Bit-identical to the
    reference. `form` ("one_workgroup" / "persistent" / "per_sample") forces one of the library's forms (sp_internal_fps),
    for tests and timing; None lets the library choose. A persistent launch whose bounded wait ran out (sp_fps_status) is
    run again at once; the library then takes the per-sample form."""
    L = _lib.lib()
    p = _dev_f32(_points_of(points), 4)
    n = p.shape[0]
    order = torch.empty(max(int(sampling_num), 1), dtype=torch.int32, device=p.device)
    flags = torch.empty(n, dtype=torch.uint8, device=p.device)
    d = torch.empty(n, dtype=torch.float32, device=p.device)
    nbytes = L.sp_fps_workspace_bytes(n, sampling_num)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=p.device)
    args = (_ptr(p), n, sampling_num, first_index, _ptr(order), _ptr(flags), _ptr(d), _ptr(ws), nbytes, _stream())
    if form is None:
        check(L.sp_farthest_point_sampling(*args))
        if L.sp_fps_status(_ptr(ws), _stream()) == _lib.SP_ERR_RUNTIME:
            check(L.sp_farthest_point_sampling(*args))
    else:
        check(L.sp_internal_fps(_lib.FPS_FORM[form], *args))
    check(L.sp_fps_status(_ptr(ws), _stream()))
    return FpsResult(order, flags, d)


def weight_check(weights):
    """sp_weight_check: (the number of weights > 0, the lowest index of a weight that is not finite or < 0, or None) — the
    checks of WeightedSamplingOperator::apply (weighted_sampling_operator.hpp:43-61) in one pass. Reads two words back."""
    w = _dev_f32(weights)
    report = torch.empty(2, dtype=torch.int32, device=w.device)
    check(_lib.lib().sp_weight_check(_ptr(w), w.numel(), _ptr(report), _stream()))
    positive, bad = (int(v) & 0xFFFFFFFF for v in report.cpu().tolist())
    return positive, (None if bad == 0xFFFFFFFF else bad)


def weighted_sample_flags(weights, u_by_rank, m):
    """sp_weighted_sample_flags: the flags (uint8 [N], 1 keep) of the m largest keys log(u) / w, u_by_rank[j] being the draw of
    the j-th positive weight (weighted_sampling_operator.hpp:67-90, ties as its heap keeps them), and the number kept. The
    C++ facade draws u from the operator's generator; here the caller hands the draws in."""
    L = _lib.lib()
    w, u = _dev_f32(weights), _dev_f32(u_by_rank)
    n = w.numel()
    if u.numel() < int((w > 0).sum()):
        raise SpError(1, "u_by_rank needs a draw for every positive weight")
    flags = torch.empty(n, dtype=torch.uint8, device=w.device)
    count = torch.empty(1, dtype=torch.int32, device=w.device)
    nbytes = L.sp_weighted_sample_workspace_bytes(n)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=w.device)
    check(L.sp_weighted_sample_flags(_ptr(w), _ptr(u), n, m, _ptr(flags), _ptr(count), _ptr(ws), nbytes, _stream()))
    return flags, int(count.item())


def uniform_fill_flags(flags, positions_sorted):
    """sp_uniform_fill_flags, in place: for every p of positions_sorted (int32 or int64, ascending) the p-th point whose flag is
    not 1 gets flag 1 (mixed_random_sampling_operator.hpp:82-99 once the host has drawn the positions). Returns flags."""
    L = _lib.lib()
    if not (flags.is_cuda and flags.dtype == torch.uint8 and flags.is_contiguous()):
        raise SpError(1, "expected a contiguous uint8 CUDA tensor")
    pos = positions_sorted.to(device=flags.device, dtype=torch.int32).contiguous()
    n = flags.numel()
    nbytes = L.sp_uniform_fill_workspace_bytes(n)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=flags.device)
    check(L.sp_uniform_fill_flags(_ptr(flags), n, _ptr(pos), pos.numel(), _ptr(ws), nbytes, _stream()))
    return flags


class Communicator:
    """sp_comm: the library's own RCCL communicator (one process per GPU). The 128-byte unique id is made by rank 0
    (sp_comm_unique_id) and handed to the other ranks through whatever channel the application has — here a
    torch.distributed broadcast over an existing process group (any backend)."""

    def __init__(self, handle, rank, world):
        self._h, self.rank, self.world = handle, rank, world

    @staticmethod
    def from_process_group(group=None, device=None):
        import torch.distributed as dist

        L = _lib.lib()
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        backend = dist.get_backend(group)
        dev = torch.device("cuda", torch.cuda.current_device()) if (device is None and backend == "nccl") else (device or "cpu")
        ident = torch.zeros(_lib.COMM_ID_BYTES, dtype=torch.uint8)
        if rank == 0:
            buf = (C.c_ubyte * _lib.COMM_ID_BYTES)()
            check(L.sp_comm_unique_id(buf))
            ident = torch.tensor(list(buf), dtype=torch.uint8)
        ident = ident.to(dev)
        dist.broadcast(ident, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        raw = bytes(ident.cpu().tolist())
        h = C.c_void_p()
        check(L.sp_comm_create(raw, rank, world, C.byref(h)))  # collective: every rank of the group gets here
        return Communicator(h, rank, world)

    def all_reduce(self, t):
        """In-place float32 sum over the ranks on the current stream (sp_allreduce_f32)."""
        check(_lib.lib().sp_allreduce_f32(self._h, _ptr(t), t.numel(), _stream()))
        return t

    def all_gather(self, send, recv):
        check(_lib.lib().sp_allgather(self._h, _ptr(send), _ptr(recv), send.numel() * send.element_size(), _stream()))
        return recv

    def __del__(self):
        try:
            if self._h:
                _lib.lib().sp_comm_destroy(self._h)
                self._h = None
        except Exception:
            pass


class Exchange:
    """Direct exchange of the per-iteration row between the ranks of a sharded alignment (sp_xchg_*, csrc/sp_xchg.h): no
    collective per iteration. `all_gather(bytes) -> list of bytes in rank order` is the caller's own channel, used once."""

    def __init__(self, rank, world, all_gather, timeout_ms=None):
        L = _lib.lib()
        h = C.c_void_p()
        check(L.sp_xchg_create(int(rank), int(world), C.byref(h)))
        self._h = h
        self.rank, self.world = int(rank), int(world)
        mine = (C.c_char * 64)()
        check(L.sp_xchg_handle(self._h, mine))
        handles = all_gather(bytes(mine))
        blob = b"".join(handles)
        assert len(blob) == 64 * self.world
        check(L.sp_xchg_connect(self._h, C.c_char_p(blob)))
        if timeout_ms is not None:
            check(L.sp_xchg_set_timeout_ms(self._h, int(timeout_ms)))

    @staticmethod
    def from_process_group(group=None, timeout_ms=None):
        import torch.distributed as dist

        rank, world = dist.get_rank(group), dist.get_world_size(group)

        def gather(b):
            out = [None] * world
            dist.all_gather_object(out, b, group=group)
            return out

        return Exchange(rank, world, gather, timeout_ms)

    def __del__(self):
        try:
            if self._h:
                _lib.lib().sp_xchg_destroy(self._h)
                self._h = None
        except Exception:
            pass


class _HashedVoxelMap:
    """What VoxelHashMap and OccupancyGridMap share: the handle of an sp_vhm_* / sp_ogm_* object (the entry points differ only in
    the prefix), settings and infos by name, clear, add_point_cloud, compute_overlap_ratio and the averaged export."""
    _PREFIX = _PARAM = _INFO = None

    def __init__(self, voxel_size, device="cuda"):
        self.device = torch.device(device)
        h = C.c_void_p()
        check(self._fn("create")(float(voxel_size), _stream(), C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if self._h:
                self._fn("destroy")(self._h)
                self._h = None
        except Exception:
            pass

    def _fn(self, name):
        return getattr(_lib.lib(), f"{self._PREFIX}_{name}")

    def _set(self, name, value):
        check(self._fn("set")(self._h, self._PARAM[name], float(value)))

    def _get(self, name):
        return float(self._fn("get")(self._h, self._PARAM[name]))

    def info(self, name):
        return int(self._fn("info")(self._h, self._INFO[name]))

    def clear(self):
        check(self._fn("clear")(self._h, _stream()))

    def add_point_cloud(self, cloud, sensor_pose=None):
        T = _T16(identity() if sensor_pose is None else sensor_pose).copy()
        n = cloud.size()
        check(self._fn("add_point_cloud")(
            self._h, _ptr(cloud.points) if n else None, _ptr(cloud.covs) if (n and cloud.has_cov()) else None,
            _ptr(cloud.rgb) if (n and cloud.has_rgb()) else None,
            _ptr(cloud.intensities) if (n and cloud.has_intensity()) else None, n, T.ctypes.data_as(C.c_void_p), _stream()))

    def compute_overlap_ratio(self, cloud, sensor_pose=None):
        T = _T16(identity() if sensor_pose is None else sensor_pose).copy()
        r = C.c_float(0.0)
        n = cloud.size()
        check(self._fn("overlap_ratio")(self._h, _ptr(cloud.points) if n else None, n, T.ctypes.data_as(C.c_void_p), C.byref(r),
                                        _stream()))
        return float(r.value)

    def _mean_rows(self, entry_point, where, *limits):
        """the voxel means `entry_point` keeps around `where` (a position, or a pose as 16 floats) within `limits` (floats), as a
        PointCloudShared, and their keys in the same order"""
        cap = self.info("voxel_num")
        dev = self.device
        rows = max(cap, 1)
        pts = torch.empty((rows, 4), dtype=torch.float32, device=dev)
        covs = torch.empty((rows, 16), dtype=torch.float32, device=dev) if self.info("has_cov") else None
        rgb = torch.empty((rows, 4), dtype=torch.float32, device=dev) if self.info("has_rgb") else None
        inten = torch.empty(rows, dtype=torch.float32, device=dev) if self.info("has_intensity") else None
        keys = torch.empty(rows, dtype=torch.int64, device=dev)
        c = np.ascontiguousarray(where, np.float32).copy()
        n_out = C.c_size_t(0)
        check(self._fn(entry_point)(self._h, c.ctypes.data_as(C.c_void_p), *[float(v) for v in limits], _ptr(pts), _ptr(covs),
                                    _ptr(rgb), _ptr(inten), _ptr(keys), cap, C.byref(n_out), _stream()))
        n = n_out.value
        out = PointCloudShared(pts[:n], covs=None if covs is None else covs[:n], rgb=None if rgb is None else rgb[:n],
                               intensities=None if inten is None else inten[:n], device=dev)
        return out, keys[:n]


class VoxelHashMap(_HashedVoxelMap):
    """algorithms/mapping/voxel_hash_map.hpp:22-250 over the sp_vhm_* entry points: submap accumulation in HBM.
    add_point_cloud takes a PointCloudShared in the sensor frame and the sensor pose (4x4, map frame); downsampling
    returns a PointCloudShared of the voxel means inside the query box (plus `.voxel_keys`, the keys in output order)."""
    _PREFIX = "sp_vhm"
    _PARAM = {"voxel_size": 0, "max_staleness": 1, "remove_old_data_cycle": 2, "rehash_threshold": 3, "min_num_point": 4}
    _INFO = {"voxel_num": 0, "capacity": 1, "staleness_counter": 2, "has_cov": 3, "has_rgb": 4, "has_intensity": 5}

    def set_voxel_size(self, v): self._set("voxel_size", v)  # noqa: E704
    def get_voxel_size(self): return self._get("voxel_size")  # noqa: E704
    def set_max_staleness(self, v): self._set("max_staleness", v)  # noqa: E704
    def get_max_staleness(self): return int(self._get("max_staleness"))  # noqa: E704
    def set_remove_old_data_cycle(self, v): self._set("remove_old_data_cycle", v)  # noqa: E704
    def get_remove_old_data_cycle(self): return int(self._get("remove_old_data_cycle"))  # noqa: E704
    def set_rehash_threshold(self, v): self._set("rehash_threshold", v)  # noqa: E704
    def get_rehash_threshold(self): return self._get("rehash_threshold")  # noqa: E704
    def set_min_num_point(self, v): self._set("min_num_point", v)  # noqa: E704
    def get_min_num_point(self): return int(self._get("min_num_point"))  # noqa: E704

    def downsampling(self, center=(0.0, 0.0, 0.0), distance=100.0):
        out, keys = self._mean_rows("downsampling", center, distance)
        out.voxel_keys = keys
        return out

    def remove_old_data(self):
        check(_lib.lib().sp_vhm_remove_old_data(self._h, _stream()))

    def prepare_registration(self, reg_type="GICP"):
        """sp_vhm_prepare_registration: the rows Registration.align_voxel_map reads, for the map as it is now (one launch)."""
        check(_lib.lib().sp_vhm_prepare_registration(self._h, REG[reg_type], _stream()))

    def registration_ready(self, reg_type="GICP"):
        return bool(_lib.lib().sp_vhm_registration_ready(self._h, REG[reg_type]))


class OccupancyGridMap(_HashedVoxelMap):
    """algorithms/mapping/occupancy_grid_map.hpp:27-190, 417 over the sp_ogm_* entry points: the log-odds submap in HBM, with
    free-space carving along the rays from the sensor. add_point_cloud takes a PointCloudShared in the sensor frame and the sensor
    pose (4x4, map frame); extract_occupied_points returns a PointCloudShared of the occupied voxels' means (plus `.keys`, the voxel
    keys in output order: rows are in table-slot order, align them by key); extract_visible_points returns, in the same form, those
    of them inside the sensor's frustum that no other occupied voxel hides."""
    _PREFIX = "sp_ogm"
    _PARAM = {"voxel_size": 0, "log_odds_hit": 1, "log_odds_miss": 2, "log_odds_min": 3, "log_odds_max": 4,
              "occupancy_threshold": 5, "free_space_updates_enabled": 6, "voxel_pruning_enabled": 7, "stale_frame_threshold": 8,
              "rehash_threshold": 9}
    _INFO = {"voxel_num": 0, "capacity": 1, "frame_index": 2, "has_cov": 3, "has_rgb": 4, "has_intensity": 5}

    def set_voxel_size(self, v): self._set("voxel_size", v)  # noqa: E704
    def voxel_size(self): return self._get("voxel_size")  # noqa: E704
    def set_log_odds_hit(self, v): self._set("log_odds_hit", v)  # noqa: E704
    def set_log_odds_miss(self, v): self._set("log_odds_miss", v)  # noqa: E704
    def set_free_space_updates_enabled(self, on): self._set("free_space_updates_enabled", bool(on))  # noqa: E704
    def set_voxel_pruning_enabled(self, on): self._set("voxel_pruning_enabled", bool(on))  # noqa: E704
    def set_occupancy_threshold(self, probability): self._set("occupancy_threshold", probability)  # noqa: E704
    def set_stale_frame_threshold(self, v): self._set("stale_frame_threshold", int(v))  # noqa: E704
    def set_rehash_threshold(self, v): self._set("rehash_threshold", v)  # noqa: E704

    def set_log_odds_limits(self, minimum, maximum):
        check(_lib.lib().sp_ogm_set_log_odds_limits(self._h, float(minimum), float(maximum)))

    def get(self, name):
        """the value of a setting by name (occupancy_threshold as a probability)"""
        return self._get(name)

    def extract_occupied_points(self, sensor_pose=None, max_distance=100.0):
        T = np.asarray(identity() if sensor_pose is None else sensor_pose, np.float32).reshape(4, 4)
        out, keys = self._mean_rows("extract_occupied_points", T[:3, 3], max_distance)
        out.keys = keys
        return out

    def extract_visible_points(self, sensor_pose, max_distance, horizontal_fov, vertical_fov):
        """occupancy_grid_map.hpp:183-411: the fields of view in radians, around the sensor's x axis"""
        out, keys = self._mean_rows("extract_visible_points", _T16(sensor_pose), max_distance, horizontal_fov, vertical_fov)
        out.keys = keys
        return out

    def voxel_probability(self, position):
        p = np.asarray(position, np.float32).reshape(-1)[:3].copy()
        r = C.c_float(0.5)
        check(_lib.lib().sp_ogm_voxel_probability(self._h, p.ctypes.data_as(C.c_void_p), C.byref(r), _stream()))
        return float(r.value)

    def export(self):
        """every live voxel in table-slot order, as numpy arrays: keys (uint64), hit_count, miss_count, log_odds, last_updated,
        sum_xyz (n, 3), cov_sums (n, 6: xx xy xz yy yz zz of the log-covariances), rgb_sums (n, 4), intensity_sums"""
        cap = self.info("voxel_num")
        dev = self.device
        rows = max(cap, 1)
        mk = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        keys, hits, miss = mk(rows, torch.int64), mk(rows, torch.int32), mk(rows, torch.int32)
        lo, last, xyz = mk(rows, torch.float32), mk(rows, torch.int32), mk((rows, 3), torch.float32)
        cov, rgb, inten = mk((rows, 6), torch.float32), mk((rows, 4), torch.float32), mk(rows, torch.float32)
        n_out = C.c_size_t(0)
        check(_lib.lib().sp_ogm_export(self._h, _ptr(keys), _ptr(hits), _ptr(miss), _ptr(lo), _ptr(last), _ptr(xyz), _ptr(cov),
                                       _ptr(rgb), _ptr(inten), cap, C.byref(n_out), _stream()))
        n = n_out.value
        host = lambda t: t[:n].cpu().numpy()  # noqa: E731
        return {"keys": host(keys).view(np.uint64), "hit_count": host(hits).view(np.uint32),
                "miss_count": host(miss).view(np.uint32), "log_odds": host(lo), "last_updated": host(last).view(np.uint32),
                "sum_xyz": host(xyz), "cov_sums": host(cov), "rgb_sums": host(rgb), "intensity_sums": host(inten)}


class PreparedTarget:
    """Plane-regularised target covariances stored in the cell order of a GridKNN (sp_gicp_target_*): the target half of
    the prepared / fused GICP iteration. Holds a reference to the grid, which it borrows."""

    def __init__(self, grid, covs, reg_type="GICP"):
        self.grid = grid
        self.covs = _dev_f32(covs, 16)
        self.reg_type = reg_type
        h = C.c_void_p()
        check(_lib.lib().sp_gicp_target_create(grid._h, _ptr(self.covs), self.covs.shape[0], _stream(), C.byref(h)))
        self._h = h
        if reg_type != "GICP":  # POINT_TO_DISTRIBUTION: the rows hold inverse(Ct) (sp_gicp_target_prepare)
            check(_lib.lib().sp_gicp_target_prepare(self._h, _ptr(self.covs), REG[reg_type], _stream()))

    def update(self, covs=None, reg_type=None):
        if covs is not None:
            self.covs = _dev_f32(covs, 16)
        if reg_type is not None:
            self.reg_type = reg_type
        check(_lib.lib().sp_gicp_target_prepare(self._h, _ptr(self.covs), REG[self.reg_type], _stream()))

    def __del__(self):
        try:
            if self._h:
                _lib.lib().sp_gicp_target_destroy(self._h)
                self._h = None
        except Exception:
            pass


class PreparedSource:
    """Prepared source of the fused GICP iteration (sp_gicp_source_*): packed plane-regularised covariances and,
    optionally, the cloud reordered by target-grid cell. Buffers are allocated once for n_max points."""

    def __init__(self, n_max):
        h = C.c_void_p()
        check(_lib.lib().sp_gicp_source_create(n_max, C.byref(h)))
        self._h = h
        self.n_max = n_max

    def _set_option(self, name, value):
        """csrc/sp_internal.h measurement / tuning switch of this prepared source (tests / bench / scratch only)."""
        check(_lib.lib().sp_internal_source_option(self._h, _lib.INTERNAL_OPTION[name], int(value)))

    def prepare(self, prepared_target, source, transT=None, sort_by_cell=True):
        p2d = getattr(prepared_target, "reg_type", "GICP") == "POINT_TO_DISTRIBUTION"  # no source covariance in that factor
        if not source.has_cov() and not p2d:
            raise SpError(2, "[Registration::validate_params] Covariance matrices of source and target must be "
                             "pre-computed before performing GICP matching.")
        tp, on_dev, keep = _trans_arg(transT)
        check(_lib.lib().sp_gicp_source_prepare(self._h, prepared_target._h, _ptr(source.points),
                                                _ptr(source.covs if source.has_cov() else None),
                                                source.size(), tp, on_dev, _SOURCE_ORDER[sort_by_cell], _stream()))
        self.n = source.size()

    def __del__(self):
        try:
            if self._h:
                _lib.lib().sp_gicp_source_destroy(self._h)
                self._h = None
        except Exception:
            pass


# ------------------------------------------------------------------ registration
@dataclass
class RegistrationParams:
    """registration_params.hpp:46-114 (defaults copied from there)."""
    reg_type: str = "GICP"
    max_correspondence_distance: float = 2.0
    robust_type: str = "NONE"
    robust_default_scale: float = 10.0
    genz_planarity_threshold: float = 0.2
    optimization_method: str = "GN"  # GN | LM
    gn_lambda: float = 1.0
    lm_max_inner_iterations: int = 10
    lm_lambda_factor: float = 2.0
    lm_init_lambda: float = 1.0
    lm_max_lambda: float = 1e3
    lm_min_lambda: float = 1e-6
    dogleg_initial_trust_region_radius: float = 1.0  # registration_params.hpp:84-92
    dogleg_min_trust_region_radius: float = 1e-4
    dogleg_max_trust_region_radius: float = 10.0
    dogleg_eta1: float = 0.25
    dogleg_eta2: float = 0.75
    dogleg_gamma_decrease: float = 0.25
    dogleg_gamma_increase: float = 2.0
    max_iterations: int = 20
    criteria_translation: float = 1e-3
    criteria_rotation: float = 1e-3
    verbose: bool = False
    # default-off terms
    rotation_constraint_enable: bool = False  # registration_params.hpp:56-64
    rotation_constraint_weight: float = 1.0
    rotation_constraint_robust_default_scale: float = 10.0
    degenerate_reg_type: str = "NONE"  # NONE | NL_REG (degenerate_regularization.hpp:41-46)
    degenerate_reg_rot_eigenvalue_threshold: float = 10.0
    degenerate_reg_trans_eigenvalue_threshold: float = 1.0
    degenerate_reg_base_factor: float = 1.0
    map_prior_enabled: bool = False  # map_prior.hpp:14-35
    map_prior_rot_vel_sigma: float = 1.0
    map_prior_trans_vel_sigma: float = 1.0
    map_prior_rot_base_sigma: float = 3.16e-2
    map_prior_trans_base_sigma: float = 1e-2
    photometric: PhotometricParams = field(default_factory=PhotometricParams)  # MI355X extension: align(target_gradients=...)


def _opt_params(p):
    """sp_opt_params of a RegistrationParams"""
    return _lib.OptParams({"GN": 0, "LM": 1, "DOGLEG": 2}[p.optimization_method], p.max_iterations, p.criteria_rotation,
                          p.criteria_translation, p.gn_lambda, p.lm_max_inner_iterations, p.lm_lambda_factor,
                          p.lm_init_lambda, p.lm_max_lambda, p.lm_min_lambda, p.dogleg_initial_trust_region_radius,
                          p.dogleg_min_trust_region_radius, p.dogleg_max_trust_region_radius, p.dogleg_eta1, p.dogleg_eta2,
                          p.dogleg_gamma_decrease, p.dogleg_gamma_increase)


@dataclass
class RegistrationResult:
    """result.hpp:12-28"""
    T: np.ndarray = field(default_factory=identity)
    converged: bool = False
    iterations: int = 0
    H: np.ndarray = field(default_factory=lambda: np.zeros((6, 6), np.float32))
    b: np.ndarray = field(default_factory=lambda: np.zeros(6, np.float32))
    error: float = FLT_MAX
    inlier: int = 0
    H_raw: np.ndarray = field(default_factory=lambda: np.zeros((6, 6), np.float32))  # before regularisation / prior
    b_raw: np.ndarray = field(default_factory=lambda: np.zeros(6, np.float32))
    error_raw: float = FLT_MAX


class Registration:
    """algorithms/registration/registration.hpp:88-965 for the GN / LM optimisers.

    align() is the reference's host-driven loop (one 192-byte read-back per iteration).
    align_device_loop() keeps pose, linear system and solve on the device for a fixed number of iterations — the
    form the benchmark times — and takes an optional torch.distributed process group: each rank linearises its shard
    of the source and the 176-byte system is summed over ranks (RCCL over xGMI) before the solve.
    """

    def __init__(self, params=None):
        self.params = params or RegistrationParams()
        self.neighbors = KNNResult()
        self._ws = None
        self._lin = None
        self.genz_alpha = 1.0
        self._rot_scale = self.params.rotation_constraint_robust_default_scale
        self._map_prior = MapPriorState()
        self._psrc = None
        self._source_options = {}  # csrc/sp_internal.h switches applied to the prepared source (tests / bench only)

    def _set_source_option(self, name, value):
        self._source_options[name] = int(value)
        if self._psrc is not None:
            self._psrc._set_option(name, value)

    def _prepared_source(self, n):
        if self._psrc is None or self._psrc.n_max < n:
            self._psrc = PreparedSource(n)
            for k, v in self._source_options.items():
                self._psrc._set_option(k, v)
            return self._psrc, True
        return self._psrc, False

    def set_map_prior_state(self, prev_result, T_pred):
        """registration.hpp:124-126 / MapPrior::update (map_prior.hpp:97-174): call once per frame, after motion
        prediction and before align(); `prev_result` is the previous frame's RegistrationResult."""
        p = self.params
        mp = MapPriorParams(int(p.map_prior_enabled), p.map_prior_rot_vel_sigma, p.map_prior_trans_vel_sigma,
                            p.map_prior_rot_base_sigma, p.map_prior_trans_base_sigma)
        Hraw = np.ascontiguousarray(prev_result.H_raw, np.float32)
        Tprev, Tpred = _T16(prev_result.T).copy(), _T16(T_pred).copy()
        check(_lib.lib().sp_map_prior_update_host(C.byref(mp), Hraw.ctypes.data_as(C.c_void_p),
                                                  C.c_float(prev_result.error_raw), int(prev_result.inlier),
                                                  Tprev.ctypes.data_as(C.c_void_p), Tpred.ctypes.data_as(C.c_void_p),
                                                  C.byref(self._map_prior)))
        return bool(self._map_prior.has_prior)

    def _prior_error(self, T16):
        if not (self.params.map_prior_enabled and self._map_prior.has_prior):
            return np.float32(0.0)
        return np.float32(_lib.lib().sp_map_prior_apply_host(C.byref(self._map_prior), T16.ctypes.data_as(C.c_void_p),
                                                             None, None, None))

    # -- helpers
    def _buffers(self, device):
        L = _lib.lib()
        if self._ws is None or self._ws.device != device:
            self._ws = torch.empty(L.sp_gicp_workspace_bytes(0), dtype=torch.uint8, device=device)
            self._lin = torch.zeros(48, dtype=torch.float32, device=device)
        return self._ws, self._lin

    def _factor_params(self, robust_scale):
        p = self.params
        return FactorParams(REG[p.reg_type], LOSS[p.robust_type], p.max_correspondence_distance, robust_scale,
                            self.genz_alpha, p.genz_planarity_threshold, int(p.rotation_constraint_enable),
                            p.rotation_constraint_weight, self._rot_scale)

    def _validate(self, source, target):
        p = self.params
        if p.reg_type == "POINT_TO_PLANE" and not target.has_normal():
            if not target.has_cov():
                raise SpError(2, "[Registration::validate_params] Normal vector or covariance matrices of target must "
                                 "be pre-computed before performing Point-to-Plane ICP matching.")
            covariance.extract_normals(target)
        if p.reg_type == "GICP" and (not source.has_cov() or not target.has_cov()):
            raise SpError(2, "[Registration::validate_params] Covariance matrices of source and target must be "
                             "pre-computed before performing GICP matching.")
        if p.reg_type == "GENZ":
            if not target.has_cov():
                raise SpError(2, "[Registration::validate_params] Covariance matrices of target must be pre-computed "
                                 "before performing GenZ-ICP matching.")
            if not target.has_normal():
                covariance.extract_normals(target)
        if p.reg_type == "POINT_TO_DISTRIBUTION" and not target.has_cov():
            raise SpError(2, "[Registration::validate_params] Covariance matrices of target must be pre-computed "
                             "before performing Point-to-Distribution ICP matching.")
        if p.rotation_constraint_enable and not source.has_cov():
            raise SpError(2, "[Registration::validate_params] Covariance matrices of source are required for "
                             "performing rotation constraint matching.")
        if p.rotation_constraint_enable and not target.has_cov():
            raise SpError(2, "[Registration::validate_params] Covariance matrices of target are required for "
                             "performing rotation constraint matching.")
        if p.robust_type != "NONE" and p.robust_default_scale <= 0.0:
            p.robust_type = "NONE"

    def _linearize(self, which, source, target, transT, robust_scale, lin):
        L = _lib.lib()
        ws, _ = self._buffers(source.points.device)
        fp = self._factor_params(robust_scale)
        tp, on_dev, keep = _trans_arg(transT)
        fn = L.sp_gicp_linearize if which == "linearize" else L.sp_gicp_error
        check(fn(_ptr(source.points), _ptr(source.covs if source.has_cov() else None), source.size(),
                 _ptr(target.points), _ptr(target.covs if target.has_cov() else None),
                 _ptr(target.normals if target.has_normal() else None), _ptr(self.neighbors.indices),
                 _ptr(self.neighbors.distances), tp, on_dev, C.byref(fp), _ptr(lin), _ptr(ws), ws.numel(), _stream()))

    def _genz_alpha(self, source, target):
        cnt = torch.zeros(2, dtype=torch.int32, device=source.points.device)
        check(_lib.lib().sp_genz_counts(_ptr(target.covs), _ptr(self.neighbors.indices), _ptr(self.neighbors.distances),
                                        source.size(), self.params.max_correspondence_distance,
                                        self.params.genz_planarity_threshold, _ptr(cnt), _stream()))
        inl, pl = [int(x) for x in cnt.cpu().tolist()]
        return 1.0 if inl == 0 else float(np.float32(pl) / np.float32(inl))

    @staticmethod
    def _read_lin(lin):
        h = lin.cpu().numpy()
        out = Linearized()
        C.memmove(C.byref(out), h.ctypes.data, 192)
        return out

    def compute_linearized_result(self, source, target, target_knn, pose, robust_scale=-1.0, rotation_robust_scale=-1.0,
                                  initial_pose=None):
        """registration.hpp:312-331; with `initial_pose` the degenerate regularisation is applied (:323)."""
        scale = robust_scale if robust_scale > 0 else self.params.robust_default_scale
        self._rot_scale = (rotation_robust_scale if rotation_robust_scale > 0
                           else self.params.rotation_constraint_robust_default_scale)
        _, lin = self._buffers(source.points.device)
        target_knn.nearest_neighbor_search_async(source, self.neighbors, pose)
        if self.params.reg_type == "GENZ":
            self.genz_alpha = self._genz_alpha(source, target)
        self._linearize("linearize", source, target, pose, scale, lin)
        r = self._read_lin(lin)
        p = self.params
        if initial_pose is not None and p.degenerate_reg_type.upper() != "NONE":
            dreg = DegenerateRegParams(1, p.degenerate_reg_rot_eigenvalue_threshold,
                                       p.degenerate_reg_trans_eigenvalue_threshold, p.degenerate_reg_base_factor)
            Tc, Ti = _T16(pose).copy(), _T16(initial_pose).copy()
            check(_lib.lib().sp_degenerate_regularize_host(C.byref(dreg), r.H, r.b, r.inlier,
                                                           Tc.ctypes.data_as(C.c_void_p), Ti.ctypes.data_as(C.c_void_p)))
        return {"H": np.array(r.H, np.float32).reshape(6, 6), "b": np.array(r.b, np.float32), "error": float(r.error),
                "inlier": int(r.inlier)}

    def compute_error_frozen(self, source, target, pose, robust_scale=-1.0, rotation_robust_scale=-1.0):
        """registration.hpp:350-359 — error at `pose` with the cached correspondences."""
        scale = robust_scale if robust_scale > 0 else self.params.robust_default_scale
        self._rot_scale = (rotation_robust_scale if rotation_robust_scale > 0
                           else self.params.rotation_constraint_robust_default_scale)
        _, lin = self._buffers(source.points.device)
        self._linearize("error", source, target, pose, scale, lin)
        r = self._read_lin(lin)
        return float(r.error), int(r.inlier)

    def compute_icp_robust_weights(self, source, target, target_knn, pose, robust_scale):
        """registration.hpp:279-294"""
        out = torch.zeros(source.size(), dtype=torch.float32, device=source.points.device)
        if source.size() == 0:
            return out
        target_knn.nearest_neighbor_search_async(source, self.neighbors, pose)
        fp = self._factor_params(robust_scale)
        tp, on_dev, keep = _trans_arg(pose)
        check(_lib.lib().sp_icp_robust_weights(
            _ptr(source.points), _ptr(source.covs if source.has_cov() else None), source.size(), _ptr(target.points),
            _ptr(target.covs if target.has_cov() else None), _ptr(target.normals if target.has_normal() else None),
            _ptr(self.neighbors.indices), _ptr(self.neighbors.distances), tp, on_dev, C.byref(fp), _ptr(out), _stream()))
        return out

    # -- the reference's host-driven loop
    def align(self, source, target, target_knn, initial_guess=None, robust_scale=-1.0, rotation_robust_scale=-1.0,
              target_gradients=None):
        """registration.hpp:201-276 with optimize_gauss_newton (:803-828) / optimize_levenberg_marquardt (:830-895) /
        optimize_powell_dogleg (:897-965); degenerate regularisation and the MAP prior act on the reduced system
        between the device reduction and the solve (:236-253).
        target_gradients (MI355X extension): intensity_gradients() of the target. With params.photometric.weight > 0 every
        linearisation adds weight x the photometric system over the same correspondences BEFORE the pose terms (the degenerate
        regulariser and the MAP prior see the combined system; H_raw / b_raw / error_raw are the combined system too), and every
        trial error adds weight x the photometric error; `inlier` stays the geometric count. With weight 0 it is ignored."""
        L = _lib.lib()
        p = self.params
        ph = p.photometric
        photo = target_gradients is not None and ph.weight > 0
        if photo:  # (before anything is enqueued)
            if not source.has_intensity():
                raise SpError(2, "[Registration::align] the photometric term needs the intensities of the source")
            if target_gradients.shape[0] != target.size():
                raise SpError(1, "[Registration::align] target_gradients has another size than the target")
        result = RegistrationResult()
        result.T = identity() if initial_guess is None else np.array(initial_guess, np.float32)
        if source.size() == 0:
            return result
        self._validate(source, target)
        scale = robust_scale if robust_scale > 0 else p.robust_default_scale
        self._rot_scale = (rotation_robust_scale if rotation_robust_scale > 0
                           else p.rotation_constraint_robust_default_scale)
        _, lin = self._buffers(source.points.device)
        T = _T16(result.T).copy().reshape(-1)  # column-major working copy

        def linearize_at(Tcol):
            Tmat = Tcol.reshape(4, 4).T
            target_knn.nearest_neighbor_search_async(source, self.neighbors, Tmat)
            if p.reg_type == "GENZ":
                self.genz_alpha = self._genz_alpha(source, target)
            self._linearize("linearize", source, target, Tmat, scale, lin)
            if not photo:
                return self._read_lin(lin)  # the reference's wait_and_throw + toCPU (registration.hpp:674-675)
            photometric_linearize(source, target.points, target_gradients, self.neighbors, Tmat, ph, p.max_correspondence_distance,
                                  lin=lin2, workspace=self._ws)
            lr, li = self._read_lin(lin), self._read_lin(lin2)
            w = np.float32(ph.weight)
            H = np.array(lr.H, np.float32) + w * np.array(li.H, np.float32)
            b = np.array(lr.b, np.float32) + w * np.array(li.b, np.float32)
            lr.H[:], lr.b[:] = H.tolist(), b.tolist()
            lr.error = np.float32(lr.error) + w * np.float32(li.error)
            return lr

        def error_at(Tcol, Tlin_col):
            Tmat = Tcol.reshape(4, 4).T
            err, inl = self.compute_error_frozen(source, target, Tmat, scale, self._rot_scale)
            if photo:
                photometric_error(source, target.points, target_gradients, self.neighbors, Tmat, ph, p.max_correspondence_distance,
                                  lin=lin2, workspace=self._ws)
                err = float(np.float32(err) + np.float32(ph.weight) * np.float32(self._read_lin(lin2).error))
            return err, inl

        lin2 = torch.zeros(48, dtype=torch.float32, device=source.points.device) if photo else None
        return self._host_loop(T, linearize_at, error_at, scale)

    def opt_params(self):
        """sp_opt_params of these RegistrationParams."""
        return _opt_params(self.params)

    def align_optimize(self, source, prepared_target, initial_guess=None, robust_scales=None, sort_by_cell=True, prepare=True,
                       enqueue_only=False):
        """Registration::align for every optimiser — and pipeline::RobustAligner's annealing levels around it (robust_scales:
        one align() per entry, each from the pose the previous one ended on) — as ONE launch and ONE read-back
        (sp_gicp_align_optimize). Returns a RegistrationResult that also carries `log` (one entry per outer iteration:
        level, iteration, trials, accepted, damping, error), `linearizations`, `trials`, `searched`; None when the launch is
        not available on this device right now or its bounded wait ran out (the caller takes its per-step loop).
        enqueue_only: returns the device tensor of the sp_align_result instead (nothing synchronised)."""
        L = _lib.lib()
        p = self.params
        n = source.size()
        dev = source.points.device
        ws, _ = self._buffers(dev)
        T0 = identity() if initial_guess is None else np.asarray(initial_guess, np.float32)
        if getattr(self, "_opt_T_dev", None) is None or self._opt_T_dev.device != dev:
            self._opt_T_dev = torch.zeros(16, dtype=torch.float32, device=dev)
            self._opt_res_dev = torch.zeros(C.sizeof(_lib.AlignResult), dtype=torch.uint8, device=dev)
            self._opt_res_host = torch.zeros(C.sizeof(_lib.AlignResult), dtype=torch.uint8).pin_memory()
        self._opt_T_dev.copy_(torch.from_numpy(_T16(T0).reshape(-1).copy()), non_blocking=True)
        psrc, _ = self._prepared_source(n)
        if prepare:
            psrc.prepare(prepared_target, source, self._opt_T_dev, sort_by_cell)
        scales = list(robust_scales) if robust_scales else [p.robust_default_scale]
        fp = self._factor_params(scales[0])
        op = self.opt_params()
        sc = (C.c_float * len(scales))(*scales)
        rc = L.sp_gicp_align_optimize(prepared_target._h, psrc._h, _ptr(self._opt_T_dev), C.byref(fp), C.byref(op), sc, len(scales),
                                      _ptr(self._opt_res_dev), _ptr(ws), ws.numel(), _stream())
        if rc == _lib.SP_ERR_RUNTIME and b"not available" in L.sp_last_error():
            return None
        check(rc)
        if enqueue_only:
            return self._opt_res_dev
        self._opt_res_host.copy_(self._opt_res_dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        r = _lib.AlignResult.from_buffer_copy(self._opt_res_host.numpy().tobytes())
        if r.status != 0:
            return None
        return self._result_from_align_result(r)

    def align_batch(self, source, prepared_target, initial_guesses, robust_scales=None, sort_by_cell=True, prepare=True):
        """MI355X extension: Registration::align of `source` against `prepared_target` from every pose of `initial_guesses`
        (a sequence of 4x4 matrices) in ONE launch, one workgroup per guess, and ONE read-back (sp_gicp_align_batch; the
        reference would call align() once per guess). The source is prepared once, at initial_guesses[0] (the order only
        decides which lane handles which point); prepare=False takes the prepared source as it is. The source's own
        correspondence cache is left alone. Returns one result per guess, each as align_optimize returns it (`log`,
        `linearizations`, `trials`, `searched`); Registration.best_of picks among them."""
        L = _lib.lib()
        p = self.params
        guesses = [np.asarray(T, np.float32) for T in initial_guesses]
        B, n = len(guesses), source.size()
        psrc, _ = self._prepared_source(n)
        if prepare:
            psrc.prepare(prepared_target, source, guesses[0] if B else None, sort_by_cell)
        scales = list(robust_scales) if robust_scales else [p.robust_default_scale]
        fp = self._factor_params(scales[0])
        op = self.opt_params()
        sc = (C.c_float * len(scales))(*scales)

        def call(T_dev, res_dev, ws):
            check(L.sp_gicp_align_batch(prepared_target._h, psrc._h, _ptr(T_dev), _ptr(T_dev), B, C.byref(fp), C.byref(op), sc,
                                        len(scales), _ptr(res_dev), _ptr(ws), ws.numel(), _stream()))

        return self._run_batch(source.points.device, guesses, L.sp_gicp_align_batch_workspace_bytes(n, B), call)

    def _run_batch(self, dev, guesses, need_bytes, call, results=None):
        """The hand-off of both batch alignments: the poses up in one copy, `call(T_dev, res_dev, ws)` (the one ctypes call: poses in
        T_dev, result blocks into res_dev — `results` when given —, a workspace of at least need_bytes), the blocks back in one
        read-back, one result per guess with its `block`. The buffers (poses | blocks | pinned blocks | workspace) are one tuple,
        _batch_bufs, grown to the largest need so far."""
        B = len(guesses)
        rsz = C.sizeof(_lib.AlignResult)
        bufs = getattr(self, "_batch_bufs", None)
        if bufs is not None and bufs[0].device != dev:
            bufs = None
        if bufs is None or bufs[0].numel() < 16 * max(B, 1) or bufs[3].numel() < need_bytes:
            slots = max(B, 1, bufs[0].numel() // 16 if bufs else 0)
            bufs = (torch.zeros(16 * slots, dtype=torch.float32, device=dev),
                    torch.zeros(rsz * slots, dtype=torch.uint8, device=dev),
                    torch.zeros(rsz * slots, dtype=torch.uint8).pin_memory(),
                    torch.empty(max(need_bytes, 16, bufs[3].numel() if bufs else 0), dtype=torch.uint8, device=dev))
            self._batch_bufs = bufs
        T_dev, res_dev, res_host, ws = bufs
        res_dev = res_dev if results is None else results
        if B:
            poses = np.stack([_T16(T).reshape(-1) for T in guesses])  # one copy up
            T_dev[:16 * B].copy_(torch.from_numpy(poses.reshape(-1).copy()), non_blocking=True)
        call(T_dev, res_dev, ws)
        res_host[:rsz * B].copy_(res_dev[:rsz * B], non_blocking=True)  # one copy down
        torch.cuda.current_stream().synchronize()
        raw = res_host[:rsz * B].numpy().tobytes()
        out = []
        for b in range(B):
            res = self._result_from_align_result(_lib.AlignResult.from_buffer_copy(raw, rsz * b))
            res.block = raw[rsz * b:rsz * (b + 1)]  # the sp_align_result as the launch wrote it
            out.append(res)
        return out

    @staticmethod
    def best_of(results):
        """Index of the best hypothesis of align_batch (sp_align_best_host): the most inliers among results with a finite pose, a
        finite error and at least one inlier; ties to the smaller error, then to the lower index. len(results) when none
        qualifies."""
        blocks = (_lib.AlignResult * max(len(results), 1))()
        for blk, r in zip(blocks, results):
            blk.T[:] = [float(v) for v in _T16(np.asarray(r.T, np.float32)).reshape(-1)]
            blk.error, blk.inlier, blk.status = float(r.error), int(r.inlier), 0
        best = C.c_size_t(len(results))
        check(_lib.lib().sp_align_best_host(C.byref(blocks), len(results), C.byref(best)))
        return int(best.value)

    def align_global(self, source, source_features, target, target_features, prepared_target, params=None, return_all=False,
                     robust_scales=None, sort_by_cell=True):
        """MI355X extension: Registration::align without an initial guess. The mutual nearest neighbours of the two clouds' FPFH
        rows (fpfh()) are the matches; params.hypotheses poses of matched triplets are scored by the matches they explain
        (sp_ransac_score), the params.guesses best become the initial guesses of align_batch against `prepared_target` (a
        PreparedTarget, or a VoxelHashMap: align_voxel_map_batch), and best_of picks the winner. Fewer than three matches, no
        hypothesis that passes its gates, or no alignment that best_of accepts: a result with converged == False and the
        identity; nothing throws. return_all: (winner, every alignment's result, the guesses as 4x4 float32). sort_by_cell: how
        align_batch prepares the source ("presorted" is what the C++ facade takes for sources of up to 4096 points). Two
        read-backs before the alignment (the match count; the scores and the matched points), one after.
        params.method == "COMPATIBILITY": the matches are every source row with its nearest target row (the mutual ones when the
        source has more than 8192 rows) and the guesses come from compat_guesses; res.hypothesis is then the winner's seed rank.
        The same early outs: nothing throws."""
        gp = params or GlobalRegistrationParams()
        none = RegistrationResult()
        done = lambda res, results=(), guesses=(): (res, list(results), list(guesses)) if return_all else res  # noqa: E731
        if source.size() == 0 or target.size() == 0 or gp.hypotheses <= 0 or gp.guesses <= 0:
            return done(none)
        compat = str(gp.method).upper() == "COMPATIBILITY"
        if not compat and str(gp.method).upper() != "TRIPLETS":
            raise SpError(1, f"[Registration::align_global] unknown method {gp.method!r}")
        if compat and source.size() <= _lib.COMPAT_MAX_MATCHES:
            # every source row with its nearest target row: the inliers that mutuality discards stay in
            idx, _ = match_features(source_features, target_features)
            corr = torch.stack([torch.arange(idx.shape[0], dtype=torch.int32, device=idx.device), idx], 1).contiguous()
        else:
            corr = match_features_mutual(source_features, target_features)
        if corr.shape[0] < 3 or (compat and corr.shape[0] > _lib.COMPAT_MAX_MATCHES):
            return done(none)
        cs, ct = correspondence_points(source, target, corr)
        if compat:
            poses, hyp = compat_guesses(cs, ct, gp)
        else:
            score = ransac_scores(cs, ct, gp.hypotheses, gp.inlier_distance, gp.min_edge, gp.edge_ratio, gp.seed)
            poses, hyp = ransac_select(score, cs, ct, gp.guesses, gp.seed)
        if len(poses) == 0:
            return done(none)
        guesses = [np.ascontiguousarray(T, np.float32) for T in poses]
        if isinstance(prepared_target, VoxelHashMap):
            results = self.align_voxel_map_batch(source, prepared_target, guesses, robust_scales)
        else:
            results = self.align_batch(source, prepared_target, guesses, robust_scales, sort_by_cell)
        best = self.best_of(results)
        if best >= len(results):
            return done(none, results, guesses)
        res = results[best]
        res.hypothesis, res.matches = int(hyp[best]), int(corr.shape[0])
        return done(res, results, guesses)

    @staticmethod
    def _result_from_align_result(r):
        res = RegistrationResult()
        res.T = np.array(r.T, np.float32).reshape(4, 4).T.copy()
        res.converged, res.iterations = bool(r.converged), int(r.iterations)
        res.H = np.array(r.H, np.float32).reshape(6, 6)
        res.b = np.array(r.b, np.float32)
        res.error, res.inlier = float(r.error), int(r.inlier)
        res.H_raw, res.b_raw, res.error_raw = res.H.copy(), res.b.copy(), float(r.error_raw)
        res.T_lin = np.array(r.T_lin, np.float32).reshape(4, 4).T.copy()
        res.linearizations, res.trials, res.searched, res.damping = int(r.linearizations), int(r.trials), int(r.searched), float(r.damping)
        res.log = [dict(level=e.level, iteration=e.iteration, trials=e.trials, accepted=e.accepted, damping=e.damping, error=e.error)
                   for e in r.log[:r.log_entries]]
        return res

    def align_prepared(self, source, prepared_target, initial_guess=None, robust_scale=-1.0, sort_by_cell=True,
                       device_resident=True):
        """Registration::align (registration.hpp:201-276) with every optimiser (GN / LM / DOGLEG) on the PREPARED path:
        each outer iteration linearises with the fused kernel (sp_gicp_iteration_fused: search or certified reuse +
        linearise + reduce), and the trial steps of LM (:830-895) and dog-leg (:897-965) evaluate the frozen-correspondence
        error with sp_gicp_error_prepared — a coalesced stream over the correspondence cache instead of the generic K12's
        gathers and two eigen-decompositions per point. GICP and POINT_TO_DISTRIBUTION (the prepared target's reg_type)."""
        L = _lib.lib()
        p = self.params
        result = RegistrationResult()
        result.T = identity() if initial_guess is None else np.array(initial_guess, np.float32)
        n = source.size()
        if n == 0:
            return result
        if p.reg_type not in ("GICP", "POINT_TO_DISTRIBUTION") or p.rotation_constraint_enable:
            raise SpError(1, "align_prepared: GICP / POINT_TO_DISTRIBUTION without the rotation constraint")
        if prepared_target.reg_type != p.reg_type:
            raise SpError(1, "align_prepared: the prepared target holds the rows of another reg_type")
        if p.robust_type != "NONE" and p.robust_default_scale <= 0.0:
            p.robust_type = "NONE"
        scale = robust_scale if robust_scale > 0 else p.robust_default_scale
        ws, lin = self._buffers(source.points.device)
        T = _T16(result.T).copy().reshape(-1)
        pose_terms = (p.degenerate_reg_type.upper() != "NONE") or (p.map_prior_enabled and bool(self._map_prior.has_prior))
        if device_resident and not pose_terms and p.max_iterations > 0:
            # the whole optimiser loop as one launch, one read-back (sp_gicp_align_optimize); the host loop below is what is
            # left for the host-side pose terms and for a device that cannot hold the launch resident
            res = self.align_optimize(source, prepared_target, result.T, [scale], sort_by_cell)
            if res is not None:
                return res
        psrc, _ = self._prepared_source(n)
        psrc.prepare(prepared_target, source, result.T, sort_by_cell)
        fp = self._factor_params(scale)

        def linearize_at(Tcol):
            check(L.sp_gicp_iteration_fused(prepared_target._h, psrc._h, Tcol.ctypes.data_as(C.c_void_p), 0, C.byref(fp), None,
                                            None, None, _ptr(lin), None, _ptr(ws), ws.numel(), _stream()))
            return self._read_lin(lin)

        def error_at(Tcol, Tlin_col):
            check(L.sp_gicp_error_prepared(prepared_target._h, psrc._h, Tlin_col.ctypes.data_as(C.c_void_p),
                                           Tcol.ctypes.data_as(C.c_void_p), 0, C.byref(fp), _ptr(lin), _ptr(ws), ws.numel(),
                                           _stream()))
            r = self._read_lin(lin)
            return float(r.error), int(r.inlier)

        return self._host_loop(T, linearize_at, error_at, scale)

    # -- voxelised GICP: the target is a VoxelHashMap (sp_vhm_linearize / sp_vhm_error)
    def _voxel_workspace(self, n, device):
        need = _lib.lib().sp_vhm_registration_workspace_bytes(n)
        ws = getattr(self, "_vws", None)
        if ws is None or ws.device != device or ws.numel() < need:
            ws = self._vws = torch.empty(need, dtype=torch.uint8, device=device)
        return ws

    def prepare_voxel_source(self, source):
        """sp_vhm_prepare_source: the packed regularised source covariances of an alignment, into this object's workspace."""
        n = source.size()
        ws = self._voxel_workspace(n, source.points.device)
        check(_lib.lib().sp_vhm_prepare_source(_ptr(source.covs if source.has_cov() else None), n, REG[self.params.reg_type], _ptr(ws),
                                               ws.numel(), _stream()))

    def linearize_voxel_map(self, source, voxel_map, pose, robust_scale=-1.0, neighbor_voxels=1, prepare_source=True,
                            want_keys=False, lin=None, workspace_bytes=None):
        """sp_vhm_linearize at `pose` (a 4x4 host matrix or 16 floats on the device): {"H", "b", "error", "inlier"} and, with
        want_keys, "keys": every source point's voxel key (int64 tensor, -1 for none). lin / workspace_bytes: the output buffer
        (48 floats on the device) and the workspace size handed to the library, for the tests of the argument checks."""
        scale = robust_scale if robust_scale > 0 else self.params.robust_default_scale
        n, dev = source.size(), source.points.device
        ws = self._voxel_workspace(n, dev)
        lin = self._buffers(dev)[1] if lin is None else lin
        if prepare_source:
            self.prepare_voxel_source(source)
        keys = torch.empty(max(n, 1), dtype=torch.int64, device=dev) if want_keys else None
        fp = self._factor_params(scale)
        tp, on_dev, keep = _trans_arg(pose)
        check(_lib.lib().sp_vhm_linearize(voxel_map._h, _ptr(source.points) if n else None, n, tp, on_dev, C.byref(fp),
                                          int(neighbor_voxels), _ptr(lin), _ptr(keys), _ptr(ws),
                                          ws.numel() if workspace_bytes is None else workspace_bytes, _stream()))
        r = self._read_lin(lin)
        out = {"H": np.array(r.H, np.float32).reshape(6, 6), "b": np.array(r.b, np.float32), "error": float(r.error),
               "inlier": int(r.inlier), "lin": r}
        if want_keys:
            out["keys"] = keys[:n]
        return out

    def error_voxel_map(self, source, voxel_map, pose, robust_scale=-1.0, lin=None, workspace_bytes=None):
        """sp_vhm_error at the trial `pose` over the correspondences the last linearize_voxel_map froze: (error, inlier)."""
        scale = robust_scale if robust_scale > 0 else self.params.robust_default_scale
        n, dev = source.size(), source.points.device
        ws = self._voxel_workspace(n, dev)
        lin = self._buffers(dev)[1] if lin is None else lin
        fp = self._factor_params(scale)
        tp, on_dev, keep = _trans_arg(pose)
        check(_lib.lib().sp_vhm_error(voxel_map._h, _ptr(source.points) if n else None, n, tp, on_dev, C.byref(fp), _ptr(lin),
                                      _ptr(ws), ws.numel() if workspace_bytes is None else workspace_bytes, _stream()))
        r = self._read_lin(lin)
        return float(r.error), int(r.inlier)

    def align_voxel_map(self, source, voxel_map, initial_guess=None, robust_scale=-1.0, neighbor_voxels=1):
        """Registration::align against a VoxelHashMap (MI355X extension): distribution-to-distribution against the Gaussian of
        the voxel each source point falls into (or of the nearest mean among 7 / 27 cells), the correspondence by hash lookup
        and no tree. The host-driven optimiser loop of align(): every optimisation method, degenerate regularisation, the MAP
        prior. The map's registration rows are refreshed here when they are not those of the map as it is now."""
        p = self.params
        result = RegistrationResult()
        result.T = identity() if initial_guess is None else np.array(initial_guess, np.float32)
        if source.size() == 0:
            return result
        if p.reg_type not in ("GICP", "POINT_TO_DISTRIBUTION") or p.rotation_constraint_enable:
            raise SpError(1, "align_voxel_map: GICP / POINT_TO_DISTRIBUTION without the rotation constraint")
        if p.reg_type == "GICP" and not source.has_cov():
            raise SpError(2, "[Registration::validate_params] Covariance matrices of source and target must be "
                             "pre-computed before performing GICP matching.")
        if p.robust_type != "NONE" and p.robust_default_scale <= 0.0:
            p.robust_type = "NONE"
        scale = robust_scale if robust_scale > 0 else p.robust_default_scale
        if not voxel_map.registration_ready(p.reg_type):
            voxel_map.prepare_registration(p.reg_type)
        self.prepare_voxel_source(source)
        T = _T16(result.T).copy().reshape(-1)

        def linearize_at(Tcol):
            return self.linearize_voxel_map(source, voxel_map, Tcol.reshape(4, 4).T, scale, neighbor_voxels, prepare_source=False)["lin"]

        def error_at(Tcol, Tlin_col):
            return self.error_voxel_map(source, voxel_map, Tcol.reshape(4, 4).T, scale)

        return self._host_loop(T, linearize_at, error_at, scale)

    def align_voxel_map_batch(self, source, voxel_map, initial_guesses, robust_scales=None, neighbor_voxels=1, want_keys=False):
        """MI355X extension: align_voxel_map from every pose of `initial_guesses` (a sequence of 4x4 matrices) in ONE launch, one
        workgroup per guess, and ONE read-back (sp_vhm_align_batch) — relocalisation against the map. The explicit call: no
        threshold, no host-side pose terms (degenerate regularisation, the MAP prior). The map's registration rows are refreshed
        here when they are not those of the map as it is now; the map itself is only read. Returns one result per guess as
        align_batch does (`log`, `linearizations`, `trials`, `searched`, `T_lin`, `block`); with want_keys each also has `keys`,
        every source point's voxel key at the last linearisation (int64 tensor, -1 for none)."""
        return self._align_voxel_map_batch(source, voxel_map, initial_guesses, robust_scales, neighbor_voxels, want_keys)

    def _align_voxel_map_batch(self, source, voxel_map, initial_guesses, robust_scales=None, neighbor_voxels=1, want_keys=False,
                               prepare=True, T_out=None, results=None, workspace_bytes=None):
        """align_voxel_map_batch with what the tests of the library's contract hand in: prepare=False takes the map's rows as they
        are; T_out / results: the output buffers; workspace_bytes: the workspace size told to the library."""
        L = _lib.lib()
        p = self.params
        guesses = [np.asarray(T, np.float32) for T in initial_guesses]
        B, n = len(guesses), source.size()
        dev = source.points.device
        if p.robust_type != "NONE" and p.robust_default_scale <= 0.0:
            p.robust_type = "NONE"
        if prepare and p.reg_type in ("GICP", "POINT_TO_DISTRIBUTION") and not voxel_map.registration_ready(p.reg_type):
            voxel_map.prepare_registration(p.reg_type)
        keys = torch.empty(max(B * n, 1), dtype=torch.int64, device=dev) if want_keys else None
        scales = list(robust_scales) if robust_scales else [p.robust_default_scale]
        fp = self._factor_params(scales[0])
        op = self.opt_params()
        sc = (C.c_float * len(scales))(*scales)

        def call(T_dev, res_dev, ws):
            check(L.sp_vhm_align_batch(voxel_map._h, _ptr(source.points) if n else None, _ptr(source.covs if source.has_cov() else None),
                                       n, _ptr(T_dev), _ptr(T_dev if T_out is None else T_out), B, C.byref(fp), C.byref(op), sc,
                                       len(scales), int(neighbor_voxels), _ptr(res_dev), _ptr(keys), _ptr(ws),
                                       ws.numel() if workspace_bytes is None else workspace_bytes, _stream()))

        out = self._run_batch(dev, guesses, L.sp_vhm_align_batch_workspace_bytes(n, B), call, results)
        if want_keys:
            for b, res in enumerate(out):
                res.keys = keys[b * n:(b + 1) * n]
        return out

    def _host_loop(self, T, linearize_at, error_at, scale):
        """The optimiser loop of Registration::align shared by the generic and the prepared path, from pose T (column-major 16
        floats): the library's stepper (sp_opt_stepper_*: the state machine of the device-resident launch) says what it wants
        next; `linearize_at(T)` returns the reduced system at pose T, `error_at(T_trial, T_lin)` the frozen-correspondence
        error."""
        L = _lib.lib()
        p = self.params
        T_initial = T.copy()
        dreg = DegenerateRegParams({"NONE": 0, "NL_REG": 1, "NL-REG": 1}[p.degenerate_reg_type.upper()],
                                   p.degenerate_reg_rot_eigenvalue_threshold,
                                   p.degenerate_reg_trans_eigenvalue_threshold, p.degenerate_reg_base_factor)
        prior_on = p.map_prior_enabled and bool(self._map_prior.has_prior)
        raw = RegistrationResult()
        op, h, req, r = self.opt_params(), C.c_void_p(), _lib.OptRequest(), _lib.AlignResult()
        check(L.sp_opt_stepper_create(C.byref(op), T.ctypes.data_as(C.c_void_p), C.byref(C.c_float(scale)), 1, C.byref(h)))
        try:
            while True:
                check(L.sp_opt_stepper_next(h, C.byref(req)))
                if req.want == _lib.OPT_WANT_DONE:
                    break
                Tq = np.array(req.T, np.float32)
                if req.want == _lib.OPT_WANT_LINEARIZE:
                    lr = linearize_at(Tq)
                    raw.H_raw = np.array(lr.H, np.float32).reshape(6, 6)  # registration.hpp:244-246
                    raw.b_raw = np.array(lr.b, np.float32)
                    raw.error_raw = float(lr.error)
                    if dreg.type:  # registration.hpp:249-250
                        check(L.sp_degenerate_regularize_host(C.byref(dreg), lr.H, lr.b, lr.inlier, Tq.ctypes.data_as(C.c_void_p),
                                                              T_initial.ctypes.data_as(C.c_void_p)))
                    if prior_on:  # registration.hpp:253
                        err = C.c_float(lr.error)
                        L.sp_map_prior_apply_host(C.byref(self._map_prior), Tq.ctypes.data_as(C.c_void_p), lr.H, lr.b, C.byref(err))
                        lr.error = err.value
                    check(L.sp_opt_stepper_linearized(h, C.byref(lr)))
                else:
                    new_error, inl = error_at(Tq, np.array(req.T_lin, np.float32))
                    new_error = np.float32(np.float32(new_error) + self._prior_error(Tq))  # registration.hpp:854, :933
                    check(L.sp_opt_stepper_trial(h, C.c_float(new_error), inl, None))
            check(L.sp_opt_stepper_result(h, C.byref(r)))
        finally:
            L.sp_opt_stepper_destroy(h)
        result = self._result_from_align_result(r)
        result.H_raw, result.b_raw, result.error_raw = raw.H_raw, raw.b_raw, raw.error_raw
        return result

    # -- device-resident fixed-length loop (GN), optionally sharded over ranks
    def align_device_loop(self, source, target, target_knn, initial_guess=None, iterations=None, robust_scale=-1.0,
                          group=None, T_dev=None, delta_dev=None):
        """`iterations` Gauss-Newton steps with no host round trip: NN(k=1) -> K11 -> [all-reduce] -> device solve.
        Returns the device tensors (T_dev 16 floats column-major, lin 48 floats, delta 8 floats); nothing is
        synchronised here."""
        import torch.distributed as dist

        L = _lib.lib()
        p = self.params
        if p.optimization_method != "GN":
            raise SpError(1, "align_device_loop implements the Gauss-Newton optimiser only")
        self._validate(source, target)
        iters = p.max_iterations if iterations is None else iterations
        scale = robust_scale if robust_scale > 0 else p.robust_default_scale
        dev = source.points.device
        _, lin = self._buffers(dev)
        if T_dev is None:
            T0 = identity() if initial_guess is None else np.asarray(initial_guess, np.float32)
            T_dev = torch.from_numpy(_T16(T0).reshape(-1).copy()).to(dev)
        if delta_dev is None:
            delta_dev = torch.zeros(8, dtype=torch.float32, device=dev)
        sharded = group is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)
        for _ in range(iters):
            target_knn.nearest_neighbor_search_async(source, self.neighbors, T_dev)
            self._linearize("linearize", source, target, T_dev, scale, lin)
            if sharded:
                dist.all_reduce(lin, op=dist.ReduceOp.SUM, group=group)  # 192 B over xGMI; latency-bound
            check(L.sp_gn_update(_ptr(lin), _ptr(T_dev), p.gn_lambda, p.criteria_rotation, p.criteria_translation,
                                 _ptr(delta_dev), _stream()))
        return T_dev, lin, delta_dev

    def align_fused_loop(self, source, prepared_target, initial_guess=None, iterations=None, robust_scale=-1.0,
                         group=None, T_dev=None, delta_dev=None, prepare=True, sort_by_cell=True,
                         write_neighbors=False, per_iteration_launches=False, update_target=False, graph=False,
                         comm=None, exchange="row", xchg=None):
        """The same fixed-length Gauss-Newton loop as align_device_loop on the prepared / fused path
        (sp_gicp_iteration_fused): one launch per iteration does NN + linearise + reduce, and, on a single GPU, the
        second (one-workgroup) launch also solves and updates the pose. On one GPU the default is
        sp_gicp_align_fused: the reduction + solve of iteration k-1 runs as the prologue of launch k, and once the
        convergence criteria hold the remaining launches return immediately (self._iters_dev holds the number of
        steps applied); per_iteration_launches=True keeps the two-launch fixed-length form. The prepared target is
        target-side pre-processing like its grid (built once by PreparedTarget(...)): pass update_target=True, or call
        prepared_target.update(covs), when the target's covariances have changed since. With prepare=True (a new alignment) the
        per-alignment preparation — plane regularisation of both clouds' covariances and the cell-order sort of the
        source at the initial pose — is enqueued first."""
        import torch.distributed as dist

        L = _lib.lib()
        p = self.params
        if p.reg_type not in ("GICP", "POINT_TO_DISTRIBUTION") or p.optimization_method != "GN":
            raise SpError(1, "align_fused_loop implements GICP / POINT_TO_DISTRIBUTION with the Gauss-Newton optimiser")
        iters = p.max_iterations if iterations is None else iterations
        scale = robust_scale if robust_scale > 0 else p.robust_default_scale
        dev = source.points.device
        ws, lin = self._buffers(dev)
        n = source.size()
        if T_dev is None:
            T0 = identity() if initial_guess is None else np.asarray(initial_guess, np.float32)
            T_dev = torch.from_numpy(_T16(T0).reshape(-1).copy()).to(dev)
        if delta_dev is None:
            delta_dev = torch.zeros(8, dtype=torch.float32, device=dev)
        if self._prepared_source(n)[1]:
            prepare = True
        if prepare:
            if update_target:
                prepared_target.update()
            self._psrc.prepare(prepared_target, source, T_dev, sort_by_cell)
        sharded = (comm is not None or group is not None or
                   (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1))
        fp = self._factor_params(scale)
        gn = GnParams(p.gn_lambda, p.criteria_rotation, p.criteria_translation)
        if xchg is not None:
            # rows exchanged directly between the ranks' buffers (sp_gicp_align_direct): one C call, no collective
            if getattr(self, "_iters_dev", None) is None or self._iters_dev.device != dev:
                self._iters_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            check(L.sp_gicp_align_direct(prepared_target._h, self._psrc._h, _ptr(T_dev), C.byref(fp),
                                         C.byref(gn), iters,
                                         xchg._h, None, None, _ptr(lin), _ptr(delta_dev), _ptr(self._iters_dev), _ptr(ws),
                                         ws.numel(), _stream()))
            self._direct_last_k = iters - 1
            return T_dev, lin, delta_dev
        if write_neighbors:
            self.neighbors.resize(n, 1, dev)
        ni = _ptr(self.neighbors.indices) if write_neighbors else None
        nd = _ptr(self.neighbors.distances) if write_neighbors else None
        if not sharded and not per_iteration_launches:
            # one C call enqueues the whole loop: one launch per iteration (+ one to finish), convergence on the device
            if getattr(self, "_iters_dev", None) is None or self._iters_dev.device != dev:
                self._iters_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            check(L.sp_gicp_align_fused(prepared_target._h, self._psrc._h, _ptr(T_dev), C.byref(fp), C.byref(gn), iters,
                                        ni, nd, _ptr(lin), _ptr(delta_dev), _ptr(self._iters_dev), _ptr(ws), ws.numel(),
                                        _stream()))
            return T_dev, lin, delta_dev
        if sharded and not per_iteration_launches:
            # one launch + one collective per iteration. exchange="row" (default): the launch reduces its partial rows to
            # ONE 128-byte row inside the kernel (fan-in, rows_all_reduced = 2) and only that row is all-reduced;
            # exchange="rows": the 32 KB of partial rows are all-reduced (round 1's form, kept for comparison). Launch k+1's
            # prologue then finishes iteration k identically on every rank. With `comm` (the library's own RCCL
            # communicator) the whole loop is ONE C call, sp_gicp_align_sharded.
            if getattr(self, "_iters_dev", None) is None or self._iters_dev.device != dev:
                self._iters_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            mode = 2 if (exchange == "row" or comm is not None) else 1
            nf = C.c_size_t(0)
            wsf = ws.view(torch.float32)
            base = ws.data_ptr()
            rows = []
            for k in (0, 1):
                fn = L.sp_gicp_align_row if mode == 2 else L.sp_gicp_align_rows
                off = (fn(_ptr(ws), k, C.byref(nf)) - base) // 4
                rows.append(wsf[off:off + nf.value])
            wsp, linp, Tp = _ptr(ws), _ptr(lin), _ptr(T_dev)

            def enqueue():
                st = _stream()
                if comm is not None:
                    check(L.sp_gicp_align_sharded(prepared_target._h, self._psrc._h, Tp, C.byref(fp), C.byref(gn), iters,
                                                  comm._h, ni, nd, linp, _ptr(delta_dev), _ptr(self._iters_dev), wsp,
                                                  ws.numel(), st))
                    return
                for k in range(iters):
                    check(L.sp_gicp_align_step(prepared_target._h, self._psrc._h, Tp, C.byref(fp), C.byref(gn), k, mode, ni, nd,
                                               linp, wsp, ws.numel(), st))
                    dist.all_reduce(rows[k & 1], op=dist.ReduceOp.SUM, group=group)
                if iters > 0:
                    check(L.sp_gicp_align_finish(self._psrc._h, _ptr(T_dev), C.byref(gn), iters - 1, mode, _ptr(lin),
                                                 _ptr(delta_dev), _ptr(self._iters_dev), _ptr(ws), ws.numel(), st))

            if not graph:
                enqueue()
                return T_dev, lin, delta_dev
            # The loop touches fixed buffers only (pose, partial rows, state), so launches + collectives of a whole
            # alignment are captured once into a hipGraph and replayed: the host then issues one launch per alignment
            # instead of 2 x iterations calls, and the GPU-side chain (kernel -> all-reduce -> kernel) is what is left.
            key = (iters, prepared_target._h.value if hasattr(prepared_target._h, "value") else id(prepared_target),
                   id(self._psrc), T_dev.data_ptr(), delta_dev.data_ptr(), ws.data_ptr(), lin.data_ptr(), ni, nd, n,
                   scale, id(group), id(comm), mode)
            graphs = self.__dict__.setdefault("_loop_graphs", {})
            g = graphs.get(key)
            if g is None:
                enqueue()  # first alignment of this shape runs eagerly (RCCL warm-up), the second one is captured
                graphs[key] = "warm"
            elif g == "warm":
                try:
                    torch.cuda.synchronize()
                    cg = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(cg):
                        enqueue()
                    graphs[key] = cg
                    cg.replay()
                except Exception as e:  # capture not supported for this collective / runtime: stay on eager launches
                    graphs[key] = False
                    import warnings
                    warnings.warn(f"align_fused_loop: hipGraph capture failed ({e!r}); using per-call launches")
                    torch.cuda.synchronize()
                    enqueue()
            elif g is False:
                enqueue()
            else:
                g.replay()
            return T_dev, lin, delta_dev
        for _ in range(iters):
            check(L.sp_gicp_iteration_fused(prepared_target._h, self._psrc._h, _ptr(T_dev), 1, C.byref(fp),
                                            None if sharded else C.byref(gn), ni, nd, _ptr(lin), _ptr(delta_dev),
                                            _ptr(ws), ws.numel(), _stream()))
            if sharded:
                dist.all_reduce(lin, op=dist.ReduceOp.SUM, group=group)
                check(L.sp_gn_update(_ptr(lin), _ptr(T_dev), p.gn_lambda, p.criteria_rotation, p.criteria_translation,
                                     _ptr(delta_dev), _stream()))
        return T_dev, lin, delta_dev

    def direct_status(self):
        """sp_gicp_align_status after align_fused_loop(..., xchg=...): raises SpError when a peer's row did not arrive."""
        ws, _ = self._buffers(torch.device("cuda", torch.cuda.current_device()))
        check(_lib.lib().sp_gicp_align_status(_ptr(ws), int(self._direct_last_k), _stream()))

    @staticmethod
    def T_from_device(T_dev):
        return T_dev.cpu().numpy().reshape(4, 4).T.copy()


# ------------------------------------------------------------------ host numerics of the odometry loop
# Thin wrappers of csrc/odometry_host.hip (the C++ facade's pipeline classes call the same entry points). Poses are 4x4 and
# rotations 3x3 row-major numpy arrays; no device is touched.
@dataclass
class AdaptiveAxisParams:
    """AdaptiveMotionPredictor::Params::AdaptiveAxis (pipeline/adaptive_motion_predictor.hpp:22-27)"""
    factor_min: float = 0.2
    factor_max: float = 1.0
    min_eigenvalue_low: float = 1.0
    min_eigenvalue_high: float = 10.0


@dataclass
class MotionPredictionParams:
    """MotionPredictor::Params (pipeline/motion_predictor.hpp:54-56, adaptive_motion_predictor.hpp:21-42)"""
    rotation: AdaptiveAxisParams = field(default_factory=lambda: AdaptiveAxisParams(min_eigenvalue_low=5.0))
    translation: AdaptiveAxisParams = field(default_factory=AdaptiveAxisParams)
    velocity_ema_alpha: float = 1.0
    mode: str = "GYRO_LIDAR_CV"

    def _c(self):
        ax = lambda a: _lib.MotionAxisParams(a.factor_min, a.factor_max, a.min_eigenvalue_low, a.min_eigenvalue_high)  # noqa: E731
        return _lib.MotionPredictParams(ax(self.rotation), ax(self.translation), self.velocity_ema_alpha,
                                        _lib.MOTION_MODE[self.mode.upper()])


class MotionPredictor:
    """MotionPredictor over AdaptiveMotionPredictor (sp_motion_predict_host); owns the velocity averages. The angular velocity is
    a rotation vector (axis * rad/s)."""

    def __init__(self, params=None):
        self.params = params or MotionPredictionParams()
        self.state = _lib.MotionPredictState()
        self.last_factors = None  # (rotation, translation) of the latest predict

    def predict(self, linear_velocity, angular_velocity, odom, dt, H_raw=None, inlier=0, registrated=False,
                gyro_delta_rotation_lidar=None, imu_se3_pose=None):
        T, f = np.zeros(16, np.float32), np.zeros(2, np.float32)
        H = None if H_raw is None else _f32(H_raw, 36)
        g = None if gyro_delta_rotation_lidar is None else _f32(np.asarray(gyro_delta_rotation_lidar, np.float32).T, 9)
        se3 = None if imu_se3_pose is None else _f32(_T16(imu_se3_pose), 16)
        check(_lib.lib().sp_motion_predict_host(C.byref(self.params._c()), C.byref(self.state), _hp(_f32(linear_velocity, 3)),
                                                _hp(_f32(angular_velocity, 3)), _hp(_f32(_T16(odom), 16)), float(dt), _hp(H),
                                                int(inlier), int(bool(registrated)), _hp(g), _hp(se3), _hp(T), _hp(f)))
        self.last_factors = (float(f[0]), float(f[1]))
        return T.reshape(4, 4).T.copy()


def velocity_from_poses(prev_pose, cur_pose, dt):
    """(linear velocity [3], angular speed, axis [3]) of prev^-1 * cur over dt (sp_velocity_from_poses_host,
    pipeline/lidar_odometry.hpp:282-286)"""
    lin, aa = np.zeros(3, np.float32), np.zeros(4, np.float32)
    check(_lib.lib().sp_velocity_from_poses_host(_hp(_f32(_T16(prev_pose), 16)), _hp(_f32(_T16(cur_pose), 16)), float(dt), _hp(lin), _hp(aa)))
    return lin, float(aa[0]), aa[1:].copy()


def keyframe_decision(last_keyframe_pose, current_pose, last_keyframe_time, timestamp, distance_threshold=2.0,
                      angle_threshold_degrees=20.0, time_threshold_seconds=1.0):
    """Submap::is_keyframe (sp_keyframe_decision_host, pipeline/submapping.hpp:144-161): (is_keyframe, distance, angle in degrees,
    delta_time)"""
    flag, m = C.c_int(0), np.zeros(3, np.float64)
    check(_lib.lib().sp_keyframe_decision_host(_hp(_f32(_T16(last_keyframe_pose), 16)), _hp(_f32(_T16(current_pose), 16)),
                                               float(last_keyframe_time), float(timestamp), float(distance_threshold),
                                               float(angle_threshold_degrees), float(time_threshold_seconds), C.byref(flag), _hp(m)))
    return bool(flag.value), float(m[0]), float(m[1]), float(m[2])


@dataclass
class InitialAlignmentParams:
    """imu::InitialAlignmentParams (algorithms/imu/imu_initial_alignment.hpp:18-46)"""
    enable: bool = True
    required_duration_sec: float = 1.0
    max_gyro_std: float = 0.01
    max_accel_std: float = 0.2
    max_accel_norm_error: float = 0.5
    estimate_gyro_bias: bool = True
    max_wait_sec: float = 5.0


@dataclass
class InitialAlignmentResult:
    """imu::InitialAlignmentResult (imu_initial_alignment.hpp:54-65)"""
    success: bool
    R_world_imu: np.ndarray
    gyro_bias: np.ndarray
    accel_mean: np.ndarray
    gyro_std: np.ndarray
    accel_std: np.ndarray
    accel_norm: float
    roll_rad: float
    pitch_rad: float
    error_message: str
    window_size: int


def estimate_initial_alignment(stamps, gyro, accel, gravity_world=(0.0, 0.0, -9.80665), params=None, current_bias=None,
                               bypass_stationarity=False):
    """imu::estimate_initial_alignment (sp_initial_alignment_host, imu_initial_alignment.hpp:85-204) on a buffer of n samples:
    stamps [n] in seconds, gyro and accel [n, 3]; current_bias is (gyro_bias, accel_bias)."""
    p = params or InitialAlignmentParams()
    t = np.ascontiguousarray(np.asarray(stamps, np.float64).reshape(-1))
    n = t.size
    ga = np.ascontiguousarray(np.concatenate([np.asarray(gyro, np.float32).reshape(n, 3), np.asarray(accel, np.float32).reshape(n, 3)], 1))
    cp = _lib.InitialAlignmentParams(p.required_duration_sec, p.max_gyro_std, p.max_accel_std, p.max_accel_norm_error,
                                     int(bool(p.estimate_gyro_bias)))
    r = _lib.InitialAlignmentResult()
    check(_lib.lib().sp_initial_alignment_host(_hp(t) if n else None, _hp(ga) if n else None, n, _hp(_f32(gravity_world, 3)), C.byref(cp),
                                               _hp(_bias6(current_bias)), int(bool(bypass_stationarity)), C.byref(r)))
    v3 = lambda f: np.array(f, np.float32)  # noqa: E731
    return InitialAlignmentResult(bool(r.success), np.array(r.R_world_imu, np.float32).reshape(3, 3).T.copy(), v3(r.gyro_bias),
                                  v3(r.accel_mean), v3(r.gyro_std), v3(r.accel_std), float(r.accel_norm), float(r.roll_rad),
                                  float(r.pitch_rad), r.error_message.decode(), int(r.window_size))


def yaw_from_rotation(R):
    """imu::detail::yaw_from_rotation (sp_yaw_from_rotation_host, imu_initial_alignment.hpp:211-218)"""
    return float(_lib.lib().sp_yaw_from_rotation_host(_hp(_f32(np.asarray(R, np.float32).T, 9))))


# ------------------------------------------------------------------ LiDAR-inertial alignment (imu/imu_factor.hpp, lio/*.hpp)
@dataclass
class IMUState:
    """imu::State (imu_factor.hpp:43-60). Error-state order [dp, dphi, dv, db_a, db_g]."""
    position: np.ndarray = field(default_factory=lambda: np.zeros(3, np.float32))
    rotation: np.ndarray = field(default_factory=lambda: np.eye(3, dtype=np.float32))
    velocity: np.ndarray = field(default_factory=lambda: np.zeros(3, np.float32))
    accel_bias: np.ndarray = field(default_factory=lambda: np.zeros(3, np.float32))
    gyro_bias: np.ndarray = field(default_factory=lambda: np.zeros(3, np.float32))
    kIdxPos, kIdxRot, kIdxVel, kIdxAccBias, kIdxGyrBias, kDOF = 0, 3, 6, 9, 12, 15

    def pack(self):
        """The 21 floats of the C ABI: p3, R9 column-major, v3, b_a3, b_g3."""
        return np.concatenate([_f32(self.position, 3), _f32(np.asarray(self.rotation, np.float32).T, 9), _f32(self.velocity, 3),
                               _f32(self.accel_bias, 3), _f32(self.gyro_bias, 3)])

    @staticmethod
    def unpack(s):
        s = np.array(s, np.float32)
        return IMUState(s[0:3].copy(), s[3:12].reshape(3, 3).T.copy(), s[12:15].copy(), s[15:18].copy(), s[18:21].copy())

    def pose(self):
        T = identity()
        T[:3, :3], T[:3, 3] = self.rotation, self.position
        return T


@dataclass
class LIORobustScheduleParams:
    """lio_registration_params.hpp:11-18"""
    auto_scale: bool = False
    init_scale: float = 10.0
    min_scale: float = 0.5
    rotation_init_scale: float = 10.0
    rotation_min_scale: float = 0.5
    auto_scaling_iter: int = 4


@dataclass
class DirectionalIcpWeightingParams:
    """lio_registration_params.hpp:28-38"""
    enable: bool = True
    trans_min_eigenvalue_per_inlier: float = 10.0
    rot_min_eigenvalue_per_inlier: float = 10.0
    trans_weak_direction_scale: float = 0.2
    rot_weak_direction_scale: float = 0.2

    def c_struct(self):
        return _lib.LioDirectionalParams(int(self.enable), self.trans_min_eigenvalue_per_inlier, self.rot_min_eigenvalue_per_inlier,
                                         self.trans_weak_direction_scale, self.rot_weak_direction_scale)


@dataclass
class RegistrationConvergenceCriteria:
    """registration_params.hpp:41-44"""
    translation: float = 1e-3
    rotation: float = 1e-3


@dataclass
class LIORegistrationParams:
    """lio_registration_params.hpp:41-49. `optimization` stands for RegistrationOptimizationParams: of the RegistrationParams only
    optimization_method and the gn / lm / dogleg fields are read."""
    total_iterations: int = 10
    criteria: RegistrationConvergenceCriteria = field(default_factory=RegistrationConvergenceCriteria)
    optimization: RegistrationParams = field(default_factory=RegistrationParams)
    robust: LIORobustScheduleParams = field(default_factory=LIORobustScheduleParams)
    invalid_regularization_factor: float = 1e4
    directional_icp_weighting: DirectionalIcpWeightingParams = field(default_factory=DirectionalIcpWeightingParams)

    def c_struct(self):
        o = _opt_params(self.optimization)
        o.max_iterations = int(self.total_iterations)
        o.crit_rotation, o.crit_translation = self.criteria.rotation, self.criteria.translation
        r = self.robust
        return _lib.LioParams(o, int(r.auto_scale), r.init_scale, r.min_scale, r.rotation_init_scale, r.rotation_min_scale,
                              int(r.auto_scaling_iter), self.invalid_regularization_factor, self.directional_icp_weighting.c_struct())


@dataclass
class LIOLinearizedResult:
    """lio_linearized_result.hpp"""
    H: np.ndarray = field(default_factory=lambda: np.zeros((15, 15), np.float32))
    b: np.ndarray = field(default_factory=lambda: np.zeros(15, np.float32))
    error_icp: float = 0.0
    error_imu: float = 0.0
    inlier: int = 0

    def _c(self):
        c = _lib.LioLinearized()
        C.memmove(c.H, _cm15(self.H).ctypes.data, 900)
        C.memmove(c.b, _f32(self.b, 15).ctypes.data, 60)
        c.error_icp, c.error_imu, c.inlier = self.error_icp, self.error_imu, int(self.inlier)
        return c

    def _take(self, c):
        self.H = np.array(c.H, np.float32).reshape(15, 15).T.copy()
        self.b = np.array(c.b, np.float32)
        self.error_icp, self.error_imu, self.inlier = float(c.error_icp), float(c.error_imu), int(c.inlier)


@dataclass
class LIORegistrationResult:
    """lio_registration_result.hpp: the state, the posterior covariance and the RegistrationResult fields align() fills."""
    state: IMUState = field(default_factory=IMUState)
    posterior_covariance: np.ndarray = field(default_factory=lambda: np.zeros((15, 15), np.float32))
    registration_result: RegistrationResult = field(default_factory=RegistrationResult)


def _cm15(M):
    """15x15 row-major numpy -> 225 floats column-major"""
    return _f32(np.asarray(M, np.float32).reshape(15, 15).T, 225)


def _lin6(icp):
    """a compute_linearized_result dict (or a Linearized) -> sp_linearized"""
    if isinstance(icp, Linearized):
        return icp
    c = Linearized()
    C.memmove(c.H, _f32(icp["H"], 36).ctypes.data, 144)
    C.memmove(c.b, _f32(icp["b"], 6).ctypes.data, 24)
    c.error, c.inlier = float(icp["error"]), int(icp["inlier"])
    return c


def compute_manifold_residual(x_pred, x_op):
    """imu::compute_manifold_residual (imu_factor.hpp:71-85)"""
    r = np.zeros(15, np.float32)
    check(_lib.lib().sp_imu_manifold_residual_host(_hp(x_pred.pack()), _hp(x_op.pack()), _hp(r)))
    return r


def compute_imu_hessian_gradient(x_pred, x_op, P_pred):
    """imu::compute_imu_hessian_gradient (imu_factor.hpp:116-141) -> (valid, H_imu, b_imu)"""
    H, b, ok = np.zeros(225, np.float32), np.zeros(15, np.float32), C.c_int(0)
    check(_lib.lib().sp_imu_hessian_gradient_host(_hp(x_pred.pack()), _hp(x_op.pack()), _hp(_cm15(P_pred)), _hp(H), _hp(b),
                                                  C.byref(ok)))
    return bool(ok.value), H.reshape(15, 15).T.copy(), b


def compute_imu_gradient(x_pred, x_op, H_imu):
    """imu::compute_imu_gradient (imu_factor.hpp:154-157)"""
    b = np.zeros(15, np.float32)
    check(_lib.lib().sp_imu_gradient_host(_hp(x_pred.pack()), _hp(x_op.pack()), _hp(_cm15(H_imu)), _hp(b)))
    return b


def add_icp_factor(result, icp, R_world_lidar, weight=1.0):
    """lio::add_icp_factor (lio_registration.hpp:94-113); `icp` as Registration.compute_linearized_result returns it"""
    c = result._c()
    check(_lib.lib().sp_lio_add_icp_factor_host(C.byref(c), C.byref(_lin6(icp)), _hp(_f32(np.asarray(R_world_lidar, np.float32).T, 9)),
                                                C.c_float(weight)))
    result._take(c)


def add_imu_factor(result, H_imu, b_imu, error=0.0):
    """lio::add_imu_factor (lio_registration.hpp:129-134)"""
    result.H = (result.H + np.asarray(H_imu, np.float32)).astype(np.float32)
    result.b = (result.b + np.asarray(b_imu, np.float32)).astype(np.float32)
    result.error_imu = float(error)


def apply_directional_icp_weighting(icp_factor, params):
    """lio::apply_directional_icp_weighting (lio_registration.hpp:144-202)"""
    c, p = icp_factor._c(), params.c_struct()
    check(_lib.lib().sp_lio_directional_weighting_host(C.byref(c), C.byref(p)))
    icp_factor._take(c)


def solve_ldlt(H, b, want_posterior=False):
    """lio::solve_ldlt (lio_registration.hpp:224-238) -> (ok, delta[, P_post])"""
    d, P, ok = np.zeros(15, np.float32), np.zeros(225, np.float32), C.c_int(0)
    check(_lib.lib().sp_lio_solve_ldlt_host(_hp(_cm15(H)), _hp(_f32(b, 15)), _hp(d), _hp(P) if want_posterior else None,
                                            C.byref(ok)))
    return (bool(ok.value), d, P.reshape(15, 15).T.copy()) if want_posterior else (bool(ok.value), d)


def retract(state, delta):
    """lio::retract (lio_registration.hpp:260-273)"""
    out = np.zeros(21, np.float32)
    check(_lib.lib().sp_lio_retract_host(_hp(state.pack()), _hp(_f32(delta, 15)), _hp(out)))
    return IMUState.unpack(out)


def imu_to_lidar_jacobian(T_imu_to_lidar, R_world_lidar):
    """lio::imu_to_lidar_jacobian (lio_registration.hpp:308-323)"""
    J = np.zeros(225, np.float32)
    check(_lib.lib().sp_lio_imu_to_lidar_jacobian_host(_hp(_T16(T_imu_to_lidar).reshape(-1)),
                                                       _hp(_f32(np.asarray(R_world_lidar, np.float32).T, 9)), _hp(J)))
    return J.reshape(15, 15).T.copy()


def _transform_covariance(P, T_imu_to_lidar, R_world_lidar, lidar_to_imu):
    out = np.zeros(225, np.float32)
    check(_lib.lib().sp_lio_transform_covariance_host(_hp(_cm15(P)), _hp(_T16(T_imu_to_lidar).reshape(-1)),
                                                      _hp(_f32(np.asarray(R_world_lidar, np.float32).T, 9)), int(lidar_to_imu), _hp(out)))
    return out.reshape(15, 15).T.copy()


def transform_covariance_imu_to_lidar(P_imu, T_imu_to_lidar, R_world_lidar):
    """lio::transform_covariance_imu_to_lidar (lio_registration.hpp:340-345)"""
    return _transform_covariance(P_imu, T_imu_to_lidar, R_world_lidar, 0)


def transform_covariance_lidar_to_imu(P_lidar, T_imu_to_lidar, R_world_lidar):
    """lio::transform_covariance_lidar_to_imu (lio_registration.hpp:366-381)"""
    return _transform_covariance(P_lidar, T_imu_to_lidar, R_world_lidar, 1)


def compute_dogleg_step(H, g, trust_region_radius):
    """registration::compute_dogleg_step<N> (dogleg_step.hpp:33-102), N = 6 or 15 -> (p, step_norm, predicted_reduction)"""
    g = np.ascontiguousarray(np.asarray(g, np.float32).reshape(-1))
    n = g.size
    Hc = np.ascontiguousarray(np.asarray(H, np.float32).reshape(n, n).T).reshape(-1)
    p, norm, pred = np.zeros(n, np.float32), C.c_float(0), C.c_float(0)
    check(_lib.lib().sp_dogleg_step_n_host(n, _hp(Hc), _hp(g), C.c_float(trust_region_radius), _hp(p), C.byref(norm), C.byref(pred)))
    return p, float(norm.value), float(pred.value)


def lio_factor_facts(params):
    """sp_lio_factor_facts of a RegistrationParams: what LIORegistration::align reads of the factor (lio_registration.hpp:412-415,
    444-445, 465-468)"""
    return _lib.LioFactorFacts(1 if params.reg_type in ("POINT_TO_PLANE", "GENZ") else 3, int(params.robust_type == "NONE"),
                               params.robust_default_scale, params.rotation_constraint_robust_default_scale)


class LIORegistration:
    """lio::LIORegistration (lio_registration.hpp:384-690): the library's stepper (sp_lio_stepper_*) decides, this class serves
    its requests from its own Registration: compute_linearized_result for LINEARIZE, compute_error_frozen for TRIAL."""

    def __init__(self, factor_params=None, params=None):
        self.factor_params = factor_params or RegistrationParams()
        self.params = params or LIORegistrationParams()
        self._registration = Registration(self.factor_params)

    def registration_backend(self):
        return self._registration

    def align(self, source, target, target_knn, predicted_state, predicted_covariance, previous_posterior_covariance,
              update_bias=True, dt=0.1, previous_pose=None):
        """lio_registration.hpp:396-648. `dt` and `previous_pose` are the reference's ExecutionOptions fields; no factor of this
        library reads them."""
        L = _lib.lib()
        reg = self._registration
        reg._validate(source, target)
        prm, facts = self.params.c_struct(), lio_factor_facts(self.factor_params)
        initial_pose = predicted_state.pose()
        h, req, res = C.c_void_p(), _lib.LioRequest(), _lib.LioResult()
        check(L.sp_lio_stepper_create(C.byref(prm), C.byref(facts), _hp(predicted_state.pack()), _hp(_cm15(predicted_covariance)),
                                      _hp(_cm15(previous_posterior_covariance)), int(bool(update_bias)), C.byref(h)))
        try:
            while True:
                check(L.sp_lio_stepper_next(h, C.byref(req)))
                if req.want == _lib.OPT_WANT_DONE:
                    break
                pose = np.array(req.T, np.float32).reshape(4, 4).T.copy()
                if req.want == _lib.OPT_WANT_LINEARIZE:
                    lin = reg.compute_linearized_result(source, target, target_knn, pose, req.robust_scale, req.rotation_robust_scale,
                                                        initial_pose=initial_pose)
                    check(L.sp_lio_stepper_linearized(h, C.byref(_lin6(lin))))
                else:
                    error, inlier = reg.compute_error_frozen(source, target, pose, req.robust_scale, req.rotation_robust_scale)
                    check(L.sp_lio_stepper_trial(h, C.c_float(error), inlier))
            check(L.sp_lio_stepper_result(h, C.byref(res)))
        finally:
            L.sp_lio_stepper_destroy(h)
        out = LIORegistrationResult()
        out.state = IMUState.unpack(res.state)
        out.posterior_covariance = np.array(res.posterior_covariance, np.float32).reshape(15, 15).T.copy()
        rr = out.registration_result
        rr.T, rr.converged, rr.iterations = out.state.pose(), bool(res.converged), int(res.iterations)
        rr.inlier, rr.error = int(res.inlier), float(res.error)
        return out


# ---- the per-frame loop of pipeline/lidar_inertial_odometry.hpp: what LidarInertialOdometryPipeline computes between its stages
def lio_bias_observable(gyro, accel, freeze_on_low_excitation=False, gyro_excitation_threshold=0.03, accel_excitation_threshold=0.3):
    """imu_bias_observable (lidar_inertial_odometry.hpp:371-393) on the window's samples, gyro and accel as (n, 3)"""
    g = np.ascontiguousarray(np.asarray(gyro, np.float32).reshape(-1, 3))
    a = np.ascontiguousarray(np.asarray(accel, np.float32).reshape(-1, 3))
    if g.shape != a.shape:
        raise SpError(1, f"gyro has {g.shape[0]} samples, accel {a.shape[0]}")
    out = C.c_int(-1)
    check(_lib.lib().sp_lio_bias_observable_host(_hp(g), _hp(a), g.shape[0], int(bool(freeze_on_low_excitation)),
                                                 C.c_float(gyro_excitation_threshold), C.c_float(accel_excitation_threshold),
                                                 C.byref(out)))
    return bool(out.value)


def lio_clamp_bias(bias, max_norm):
    """clamp_bias_norm (lidar_inertial_odometry.hpp:396-400) -> the clamped copy"""
    b = _f32(bias, 3).copy()
    check(_lib.lib().sp_lio_clamp_bias_host(_hp(b), C.c_float(max_norm)))
    return b


def lio_predict_state(state, T_imu_to_lidar, T_imu_rel, Delta_v, dt_total, gravity=(0.0, 0.0, -9.80665)):
    """predict_state (lidar_inertial_odometry.hpp:432-459) from the integrator's predict_relative_transform and get_corrected"""
    out = np.zeros(21, np.float32)
    check(_lib.lib().sp_lio_predict_state_host(_hp(state.pack()), _hp(_T16(T_imu_to_lidar).reshape(-1)), _hp(_T16(T_imu_rel).reshape(-1)),
                                               _hp(_f32(Delta_v, 3)), C.c_float(dt_total), _hp(_f32(gravity, 3)), _hp(out)))
    return IMUState.unpack(out)


def lio_reset_covariance(P_post, fd_velocity_sigma, icp_rotation_sigma, T_imu_to_lidar, R_world_lidar):
    """what reset_imu_preintegration (lidar_inertial_odometry.hpp:402-426) hands to the integrator -> (P_initial_imu, R_world_imu)"""
    P, R = np.zeros(225, np.float32), np.zeros(9, np.float32)
    check(_lib.lib().sp_lio_reset_covariance_host(_hp(_cm15(P_post)), C.c_float(fd_velocity_sigma), C.c_float(icp_rotation_sigma),
                                                  _hp(_T16(T_imu_to_lidar).reshape(-1)),
                                                  _hp(_f32(np.asarray(R_world_lidar, np.float32).T, 9)), _hp(P), _hp(R)))
    return P.reshape(15, 15).T.copy(), R.reshape(3, 3).T.copy()


# ------------------------------------------------------------------ sensor_msgs/PointCloud2 (ros2/convert.hpp, ros2/enhanced_reflectivity.hpp)
def _pc2_type(t):
    return _lib.PC2_TYPE[t] if isinstance(t, str) else int(t)


def _pc2_bytes(data, device="cuda"):
    """the message's bytes as a uint8 CUDA tensor: a device tensor as it is, anything else (bytes, numpy) uploaded"""
    if isinstance(data, torch.Tensor):
        if not (data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()):
            raise SpError(1, "expected a contiguous uint8 CUDA tensor")
        return data.reshape(-1)
    return torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy() if isinstance(data, (bytes, bytearray, memoryview))
                            else np.ascontiguousarray(data).view(np.uint8).reshape(-1)).to(device)


def resolve_pointcloud2_fields(fields, point_step, convert_rgb=True, convert_intensity=True, use_reflectivity_as_intensity=True):
    """fromROS2msg's field resolution (sp_pc2_resolve_fields_host, ros2/convert.hpp:38-136). fields: (name, offset, datatype)
    triples, the datatype a sensor_msgs/PointField code or its name ("FLOAT32"). Returns the _lib.Pc2Layout; SpError code 2 where
    the reference returns false, code 1 for a field that runs past point_step."""
    fields = list(fields)
    nf = len(fields)
    names = (C.c_char_p * max(nf, 1))(*[str(f[0]).encode() for f in fields])
    offsets = (C.c_uint32 * max(nf, 1))(*[int(f[1]) for f in fields])
    types = (C.c_uint8 * max(nf, 1))(*[_pc2_type(f[2]) for f in fields])
    layout = _lib.Pc2Layout()
    check(_lib.lib().sp_pc2_resolve_fields_host(names, offsets, types, nf, int(point_step), int(bool(convert_rgb)),
                                                int(bool(convert_intensity)), int(bool(use_reflectivity_as_intensity)), C.byref(layout)))
    return layout


def from_pointcloud2(data, fields, point_step, stamp=(0, 0), num_points=None, convert_rgb=True, convert_intensity=True,
                     use_reflectivity_as_intensity=True, is_bigendian=False):
    """ros2::fromROS2msg (ros2/convert.hpp:34-320) on a message given by its parts: `data` the records (a uint8 CUDA tensor is used
    where it is; bytes or numpy are uploaded), `fields` (name, offset, datatype) triples, `stamp` the header's (sec, nanosec),
    num_points = width * height (default: all whole records of data). One sp_pc2_unpack fills points, rgb, intensities and
    timestamp_offsets; start_time_ms is the stamp and end_time_ms = start_time_ms + the largest offset (one 8-byte read-back).
    None where the reference returns false (no or unsupported x / y / z) and for a big-endian message, which the reference
    misreads. An empty message gives an empty cloud."""
    if is_bigendian:
        print("Not supported big-endian point cloud", file=sys.stderr)
        return None
    try:
        layout = resolve_pointcloud2_fields(fields, point_step, convert_rgb, convert_intensity, use_reflectivity_as_intensity)
    except SpError as e:
        if e.code != _lib.SP_ERR_RUNTIME:
            raise
        print(_lib.lib().sp_last_error().decode(), file=sys.stderr)
        return None
    buf = _pc2_bytes(data)
    n = int(buf.numel()) // int(point_step) if num_points is None else int(num_points)
    dev = buf.device
    cloud = PointCloudShared(device=dev)
    cloud.start_time_ms = cloud.end_time_ms = 0.0
    if n == 0:
        return cloud
    layout.start_time_ms = float(stamp[0]) * 1000.0 + float(stamp[1]) * 1e-6
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    cloud.points = new(n, 4)
    if layout.rgb_offset >= 0:
        cloud.rgb = new(n, 4)
    if layout.intensity_offset >= 0:
        cloud.intensities = new(n)
    max_ms = ws = None
    L = _lib.lib()
    if layout.timestamp_offset >= 0:
        cloud.timestamp_offsets = new(n)
        max_ms = torch.empty(1, dtype=torch.float64, device=dev)
        ws = torch.empty(max(L.sp_pc2_unpack_workspace_bytes(n), 16), dtype=torch.uint8, device=dev)
    check(L.sp_pc2_unpack(_ptr(buf), int(buf.numel()), n, C.byref(layout), _ptr(cloud.points), _ptr(cloud.rgb),
                          _ptr(cloud.intensities), _ptr(cloud.timestamp_offsets), _ptr(max_ms), _ptr(ws), _stream()))
    if max_ms is not None:
        cloud.start_time_ms = layout.start_time_ms
        cloud.end_time_ms = cloud.start_time_ms + float(max_ms.item())
    return cloud


def to_pointcloud2(cloud):
    """ros2::toROS2msg (ros2/convert.hpp:331-429) without the message type: (data, fields, point_step) with data a uint8 CUDA
    tensor of cloud.size() records packed by sp_pc2_pack and fields (name, offset, datatype, count) tuples. The `timestamp`
    field is declared where its data is (the reference declares it 4 bytes further), so from_pointcloud2 reads it back."""
    n = cloud.size()
    has_rgb, has_int, has_ts = cloud.has_rgb(), cloud.has_intensity(), cloud.has_timestamps()
    T = _lib.PC2_TYPE
    fields = [("x", 0, T["FLOAT32"], 1), ("y", 4, T["FLOAT32"], 1), ("z", 8, T["FLOAT32"], 1)]
    offset = 16
    for name, present, dtype, size in (("rgb", has_rgb, "UINT32", 4), ("intensity", has_int, "FLOAT32", 4),
                                       ("timestamp", has_ts, "FLOAT64", 8)):
        if present:
            fields.append((name, offset, T[dtype], 1))
            offset += size
    step = int(_lib.lib().sp_pc2_pack_point_step(int(has_rgb), int(has_int), int(has_ts)))
    assert step == offset
    data = torch.empty(n * step, dtype=torch.uint8, device=cloud.points.device)
    if n:
        check(_lib.lib().sp_pc2_pack(_ptr(_dev_f32(cloud.points, 4)), _ptr(_dev_f32(cloud.rgb, 4)) if has_rgb else None,
                                     _ptr(_dev_f32(cloud.intensities)) if has_int else None,
                                     _ptr(_dev_f32(cloud.timestamp_offsets)) if has_ts else None, n,
                                     float(getattr(cloud, "start_time_ms", 0.0)), _ptr(data), _stream()))
    return data, fields, step


class EnhancedReflectivityCorrector:
    """ros2::EnhancedReflectivityCorrector (ros2/enhanced_reflectivity.hpp:32-194): range and ambient compensation of an Ouster
    scan's intensity, normalised per ring by means that are kept across scans (EMA). The means live on the device
    (`state`: 256 ref means, 256 amb means, 256 initialised flags) and sp_enhanced_reflectivity never reads anything back."""

    MAX_RINGS = _lib.ER_MAX_RINGS

    def __init__(self, ema_alpha=0.5):
        self.ema_alpha = float(ema_alpha)
        self.state = None
        self._fields = None  # (ring_offset, ring_is_u8, ambient_offset), parsed once (:145-175)

    def set_ema_alpha(self, alpha):
        self.ema_alpha = float(alpha)

    def _parse_fields(self, fields):
        if self._fields is not None:
            return True
        ambient = ring = None
        for f in fields:
            if f[0] == "ambient":
                ambient = (int(f[1]), _pc2_type(f[2]))
            elif f[0] == "ring":
                ring = (int(f[1]), _pc2_type(f[2]))
        T = _lib.PC2_TYPE
        if ambient is None or ring is None or ambient[1] != T["UINT16"] or ring[1] not in (T["UINT8"], T["UINT16"]):
            return False
        self._fields = (ring[0], ring[1] == T["UINT8"], ambient[0])
        return True

    def apply(self, cloud, data, fields, point_step, clip_max=5.0):
        """apply(cloud, msg, clip_max) (:45-140) with the message given by its parts; `data` as for from_pointcloud2 (hand it the
        tensor from_pointcloud2 was given and nothing is uploaded). False, the cloud untouched, without intensities or without an
        `ambient` (UINT16) and a `ring` (UINT8 / UINT16) field."""
        if not cloud.has_intensity() or not self._parse_fields(fields):
            return False
        n = cloud.size()
        buf = _pc2_bytes(data, cloud.points.device)
        if n * int(point_step) > buf.numel():
            raise SpError(1, "[EnhancedReflectivityCorrector] the message holds fewer records than the cloud has points")
        dev = cloud.points.device
        if self.state is None:
            self.state = torch.zeros(_lib.ER_STATE_BYTES // 4, dtype=torch.int32, device=dev)
        L = _lib.lib()
        ws = torch.empty(max(L.sp_enhanced_reflectivity_workspace_bytes(n), 16), dtype=torch.uint8, device=dev)
        ring_offset, ring_is_u8, ambient_offset = self._fields
        check(L.sp_enhanced_reflectivity(_ptr(_dev_f32(cloud.points, 4)), _ptr(_dev_f32(cloud.intensities)), n, _ptr(buf),
                                         int(point_step), ring_offset, int(ring_is_u8), ambient_offset, _ptr(self.state),
                                         self.ema_alpha, float(clip_max), _ptr(ws), _stream()))
        return True
